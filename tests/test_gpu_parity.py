"""GPU parity tests proper: every call goes through the C ABI (include/polymath_hip.h, ctypes) and is
compared bit-for-bit with the committed golden vectors (from oracle/pyref) and with the C++ CPU
restatement on the same seeded inputs; at full sizes, size-independent properties are checked.
All arithmetic is integer: the bar is exact equality."""
import numpy as np
import pytest

from helpers import BASE_NAMES, I, PT, load_golden, pm_csrs, r1cs_from_json, rand_fr_limbs
from oracle import driver as DR
from oracle.pyref import circuits as CI, serialize as SE, transcripts as T
from oracle.pyref.fields import CURVES

pytestmark = pytest.mark.gpu

CURVE_LIST = ["bls12_381", "bn254"]


@pytest.fixture(scope="module")
def api():
    from polymath_amd import api as _api
    return _api


# ------------------------------------------------------------------------------------ NTT
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_ntt_golden(gpu_ctx, oracle, curve):
    for t in load_golden("ntt_msm.json")[curve]["ntt"]:
        inp = oracle.fr_to_mont_limbs(curve, [I(x) for x in t["input"]])
        assert oracle.fr_from_mont_limbs(curve, gpu_ctx.ntt(curve, inp, t["log_n"], False)) == [I(x) for x in t["fwd"]]
        assert oracle.fr_from_mont_limbs(curve, gpu_ctx.ntt(curve, inp, t["log_n"], True)) == [I(x) for x in t["inv"]]


@pytest.mark.parametrize("curve", CURVE_LIST)
@pytest.mark.parametrize("log_n", [1, 4, 7, 8, 9, 11, 12, 13, 16, 17, 18, 19, 20])
def test_ntt_vs_oracle(gpu_ctx, oracle, curve, log_n):
    a = rand_fr_limbs(curve, 1 << log_n, 100 + log_n)
    for inverse in (False, True):
        assert np.array_equal(gpu_ctx.ntt(curve, a, log_n, inverse), oracle.ntt(curve, a, log_n, inverse, 8))


def test_ntt_full_size_roundtrip_and_domain_limit(gpu_ctx, api):
    curve, log_n = "bls12_381", 22          # the 2n transform of the 2^20 config (prover.rs:316-319)
    a = rand_fr_limbs(curve, 1 << log_n, 7)
    f = gpu_ctx.ntt(curve, a, log_n, False)
    assert not np.array_equal(f, a)
    assert np.array_equal(gpu_ctx.ntt(curve, f, log_n, True), a)
    with pytest.raises(api.PolymathError) as e:      # BN254 two-adicity 28
        gpu_ctx.ntt("bn254", np.zeros((2, 4), dtype=np.uint64), 29, False)
    assert e.value.status == 3


def test_ntt_2p25_nine_stage_passes(gpu_ctx, oracle):
    """Domains above 2^24 run 9-stage passes (512 x 4 tiles): the n = 2^25 domain of the 2^24-constraint config.
    Random round trip, and the transform of a unit vector e_j is the geometric sequence w^(jk) (checked at random
    k against big-integer powers): every butterfly's twiddle takes part."""
    curve, log_n = "bls12_381", 25
    c = CURVES[curve]
    n = 1 << log_n
    a = rand_fr_limbs(curve, n, 31)
    f = gpu_ctx.ntt(curve, a, log_n, False)
    assert np.array_equal(gpu_ctx.ntt(curve, f, log_n, True), a)
    del f
    j = 12345677
    e = np.zeros((n, 4), dtype=np.uint64)
    e[j] = oracle.fr_to_mont_limbs(curve, [1])[0]
    f = gpu_ctx.ntt(curve, e, log_n, False)
    w = pow(c.two_adic_root, 1 << (c.two_adicity - log_n), c.r)
    rng = np.random.default_rng(5)
    ks = [0, 1, n - 1, n // 2] + [int(v) for v in rng.integers(0, n, size=60)]
    want = oracle.fr_to_mont_limbs(curve, [pow(w, j * k % n, c.r) for k in ks])
    assert np.array_equal(f[ks], want)


# ------------------------------------------------------------------------------------ MSM
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_msm_golden_edge_cases(gpu_ctx, oracle, curve):
    """infinity base, zero scalar, scalar 1, scalar -1, a repeated (base, scalar) pair."""
    for t in load_golden("ntt_msm.json")[curve]["msm"]:
        bases = oracle.g1_to_mont_limbs(curve, [PT(p) for p in t["bases"]])
        sc = oracle.fr_to_mont_limbs(curve, [I(s) for s in t["scalars"]])
        out, inf = gpu_ctx.msm(curve, bases, sc)
        assert oracle.g1_from_mont_limbs(curve, out, [inf])[0] == PT(t["result"])


def test_msm_empty_and_all_zero(gpu_ctx, oracle):
    curve = "bls12_381"
    out, inf = gpu_ctx.msm(curve, np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))
    assert inf == 1 and not out.any()
    bases = oracle.g1_multiples(curve, 5)
    out, inf = gpu_ctx.msm(curve, bases, np.zeros((5, 4), dtype=np.uint64))
    assert inf == 1 and not out.any()


@pytest.mark.parametrize("curve", CURVE_LIST)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 1 << 14])
def test_msm_vs_oracle_sizes(gpu_ctx, oracle, api, curve, n):
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    host_bases = bases.download()
    assert np.array_equal(host_bases, oracle.g1_multiples(curve, n))   # device generator == CPU running sum
    sc = rand_fr_limbs(curve, n, 200 + n)
    out, inf = bases.msm(sc)
    ref, rinf = oracle.msm(curve, host_bases, sc, 8)
    assert inf == rinf == 0 and np.array_equal(out, ref)
    assert oracle.g1_is_on_curve(curve, out)


@pytest.mark.parametrize("curve", CURVE_LIST)
@pytest.mark.parametrize("n", [1, 40, 5000, 1 << 16])
def test_msm_window_tables_vs_oracle(gpu_ctx, oracle, api, curve, n):
    """pm_bases_precompute: window tables 2^(c w) P_i, single bucket set, two-level counting sort --
    same canonical result as the per-window path and as the CPU oracle (incl. offset sub-ranges)."""
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    hb = bases.download()
    sc = rand_fr_limbs(curve, n, 300 + n)
    if n >= 40:
        sc[3] = 0
        sc[4] = oracle.fr_to_mont_limbs(curve, [1])[0]
        sc[5] = oracle.fr_to_mont_limbs(curve, [CURVES[curve].r - 1])[0]
    plain, _ = bases.msm(sc)
    bases.precompute()
    assert np.array_equal(bases.download(), hb)            # window 0 is still the base vector
    tabled, inf = bases.msm(sc)
    ref, rinf = oracle.msm(curve, hb, sc, 8)
    assert inf == rinf and np.array_equal(tabled, ref) and np.array_equal(plain, ref)
    if n >= 5000:
        sub, _ = bases.msm(sc[100:3100], offset=777)
        ref, _ = oracle.msm(curve, hb[777:777 + 3000], sc[100:3100], 8)
        assert np.array_equal(sub, ref)
        same = np.repeat(sc[7:8], n, axis=0)               # one hot bucket in every window
        out, _ = bases.msm(same)
        ref, _ = oracle.msm(curve, hb, same, 8)
        assert np.array_equal(out, ref)


def test_msm_arkworks_stride_with_infinity_byte(gpu_ctx, oracle):
    """G1Affine as arkworks lays it out: x || y || infinity: bool, stride 104."""
    curve, n = "bls12_381", 50
    packed = oracle.g1_multiples(curve, n)
    wide = np.zeros((n, 13), dtype=np.uint64)
    wide[:, :12] = packed
    wide[7, 12] = 1                      # infinity flag set while coordinates are garbage
    wide[7, :12] = packed[3]
    sc = rand_fr_limbs(curve, n, 5)
    ref_b = packed.copy()
    ref_b[7] = 0
    out, inf = gpu_ctx.msm(curve, wide, sc)
    ref, _ = oracle.msm(curve, ref_b, sc, 2)
    assert np.array_equal(out, ref)


def test_msm_skewed_scalars_hot_buckets(gpu_ctx, oracle, api):
    """The reference's bench circuit makes every padding witness the same value (benches/bench.rs:49-51):
    one bucket per window receives almost every point -> exercises the task splitting."""
    curve, n = "bls12_381", 1 << 14
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    hb = bases.download()
    one_val = rand_fr_limbs(curve, 1, 9)
    sc = np.repeat(one_val, n, axis=0)
    sc[::97] = rand_fr_limbs(curve, len(sc[::97]), 10)
    out, _ = bases.msm(sc)
    ref, _ = oracle.msm(curve, hb, sc, 8)
    assert np.array_equal(out, ref)
    small = oracle.fr_to_mont_limbs(curve, [i % 3 for i in range(n)])       # booleans / tiny values
    out, _ = bases.msm(small)
    ref, _ = oracle.msm(curve, hb, small, 8)
    assert np.array_equal(out, ref)


def test_msm_hot_bucket_fold_tiers(gpu_ctx, oracle, api):
    """One repeated scalar over 2^18 pairs: a hot bucket per window owns thousands of task partials, which the
    reduction folds in parallel (msm.hip: k_task_fold, one workgroup per bucket above 1024 tasks, one wave above
    8) instead of adding them on one lane (268 ms at 2^20 before).  Per-window pipeline and window tables; a
    second, smaller repeated value lands in the wave tier."""
    curve, n = "bls12_381", 1 << 18
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    hb = bases.download()
    vals = rand_fr_limbs(curve, 2, 21)
    sc = np.repeat(vals[:1], n, axis=0)
    sc[1::5] = vals[1]                                   # ~52 K copies of a second value
    sc[::1013] = rand_fr_limbs(curve, len(sc[::1013]), 22)
    ref, _ = oracle.msm(curve, hb, sc, 8)
    out, _ = bases.msm(sc)
    assert np.array_equal(out, ref)
    bases.precompute()
    out, _ = bases.msm(sc)
    assert np.array_equal(out, ref)


def test_msm_full_size_linearity(gpu_ctx, oracle, api):
    """2^20 pairs (too slow for the CPU restatement in a unit test): MSM(s) + MSM(t) == MSM(s + t),
    and a sub-range agrees with the CPU on its own."""
    curve, n = "bls12_381", 1 << 20
    r = CURVES[curve].r
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    s, t = rand_fr_limbs(curve, n, 11), rand_fr_limbs(curve, n, 12)
    # s + t in Montgomery form == Montgomery of the sum: add as integers mod r on the host
    to_int = lambda a: [sum(int(a[i, k]) << (64 * k) for k in range(4)) for i in range(a.shape[0])]
    si, ti = to_int(s), to_int(t)
    st = oracle.ints_to_limbs([(x + y) % r for x, y in zip(si, ti)], 4)
    ps, _ = bases.msm(s)
    pt, _ = bases.msm(t)
    pst, _ = bases.msm(st)
    both, _ = gpu_ctx.g1_sum(curve, np.stack([ps, pt]))
    assert np.array_equal(both, pst)
    ref_sum, _ = oracle.g1_sum(curve, np.stack([ps, pt]))          # pm_g1_sum (host glue) vs oracle
    assert np.array_equal(both, ref_sum)
    sub, _ = bases.msm(s[1000:1000 + 4096], offset=1000)
    ref, _ = oracle.msm(curve, bases.download(1000, 4096), s[1000:1000 + 4096], 8)
    assert np.array_equal(sub, ref)


# ---------------------------------------------------------------------------- setup + prove
def _gpu_pk(api, ctx, curve, q, x, z, oracle, **kw):
    A, B, C = pm_csrs(curve, q)
    return api.ProvingKey.generate(ctx, curve, q.m0, q.mw, q.nr, A, B, C, oracle.fr_to_mont_limbs(curve, [x])[0],
                                   oracle.fr_to_mont_limbs(curve, [z])[0], **kw)


def test_golden_setup_prove_bytes(gpu_ctx, oracle, api):
    """Every committed fixture: GPU setup bases, every intermediate vector, and the 176-byte proofs for
    the three transcripts (tests/dummy.rs:75-80 shape) equal the big-integer restatement's."""
    for fx in load_golden("proofs.json") + load_golden("proofs_bn254.json"):
        curve = fx["curve"]
        c = CURVES[curve]
        TR = T.make_transcripts(c)
        q = r1cs_from_json(fx["r1cs"])
        pk = _gpu_pk(api, gpu_ctx, curve, q, I(fx["x_trapdoor"]), I(fx["z_trapdoor"]), oracle)
        assert (pk.n, pk.sigma) == (fx["n"], fx["sigma"])
        assert oracle.fr_from_mont_limbs(curve, pk.omega_limbs)[0] == I(fx["omega"])
        for i, nm in enumerate(BASE_NAMES):
            assert oracle.g1_from_mont_limbs(curve, pk.export_bases(i)) == [PT(p) for p in fx["bases"][nm]], (fx["name"], nm)
        inst, wit, r_a = [I(v) for v in fx["instance"]], [I(v) for v in fx["witness"]], [I(v) for v in fx["r_a"]]
        for tname, ref in fx["proofs"].items():
            tr = {}
            proof = DR.prove(pk, pk.n, pk.sigma, I(fx["omega"]), inst, wit, r_a, TR[tname], tr)
            assert SE.ser_proof(c, proof).hex() == ref["bytes"], (fx["name"], tname)
            if tname != "keccak256":
                continue
            for which, key in [(0, "u_evals"), (1, "w_evals"), (2, "u"), (3, "w"), (4, "h"), (5, "wit_u"), (6, "z_tail"), (7, "quotient")]:
                got = oracle.fr_from_mont_limbs(curve, pk.tap(which, 1 << 16))
                want = [I(v) for v in fx["trace"][key]]
                assert got[:len(want)] == want and not any(got[len(want):]), (fx["name"], key)
        pk.free()


def _prove_both(api, gpu_ctx, oracle, curve, q, inst, wit, seed, compare_bases=True, **gpu_kw):
    c = CURVES[curve]
    TR = T.make_transcripts(c)
    g = CI.SplitMix64(seed)
    x, z, r_a = g.fr(c.r), g.fr(c.r), [g.fr(c.r), g.fr(c.r)]
    opk = oracle.OraclePk(curve, q, x, z, 8)
    gpk = _gpu_pk(api, gpu_ctx, curve, q, x, z, oracle, **gpu_kw)
    if compare_bases:
        for i in range(6):
            assert np.array_equal(gpk.export_bases(i), opk.export_bases(i)), BASE_NAMES[i]
    omega = oracle.fr_from_mont_limbs(curve, opk.omega_limbs)[0]
    tr_o, tr_g = {}, {}
    po = DR.prove(opk, opk.n, opk.sigma, omega, inst, wit, r_a, TR["merlin"], tr_o)
    pg = DR.prove(gpk, gpk.n, gpk.sigma, omega, inst, wit, r_a, TR["merlin"], tr_g)
    assert pg == po and tr_g == tr_o
    for which in range(8):   # same vectors; the two sides may differ in trailing zero padding only
        a, b = gpk.tap(which, 1 << 22), opk.tap(which, 1 << 22)
        k = min(len(a), len(b))
        assert k > 0 and np.array_equal(a[:k], b[:k]) and not a[k:].any() and not b[k:].any(), which
    return opk, gpk, pg


@pytest.mark.parametrize("curve", CURVE_LIST)
@pytest.mark.parametrize("tables", ["1", "0"])
def test_prove_synthetic_mid_size_vs_oracle(gpu_ctx, oracle, api, curve, tables, monkeypatch):
    """SURVEY.md §8d synthetic R1CS, 3000 gates -> n = 8192, both curves; with the key's window tables
    (default) and with PM_OPT_TABLES = off (per-window Pippenger)."""
    gpu_ctx.set_option("tables", {"1": "auto", "0": "off"}[tables])       # restored by conftest
    q, inst, wit = CI.synthetic_r1cs(CURVES[curve], 3000)
    _prove_both(api, gpu_ctx, oracle, curve, q, inst, wit, 77)


def test_prove_mimc_322_vs_oracle_and_pairing(gpu_ctx, oracle, api):
    """BASELINE configs[0] shape (tests/mimc.rs): MiMC-322, n = 2048, 27 948 MSM pairs; the GPU proof
    equals the CPU restatement's and the pairing verifier accepts it."""
    from oracle.pyref import pairing as PA, protocol as PR
    from oracle.pyref.fields import BLS12_381 as c
    g = CI.SplitMix64(322)
    consts = [g.fr(c.r) for _ in range(322)]
    q, inst, wit = CI.mimc_circuit(c, g.fr(c.r), g.fr(c.r), consts)
    opk, gpk, proof = _prove_both(api, gpu_ctx, oracle, "bls12_381", q, inst, wit, 323)
    gg = CI.SplitMix64(323)
    x, z = gg.fr(c.r), gg.fr(c.r)
    omega = oracle.fr_from_mont_limbs("bls12_381", opk.omega_limbs)[0]
    from oracle.pyref.fields import BLS12_381_G2
    vk = dict(n=opk.n, m0=2, sigma=opk.sigma, omega=omega, one_g1=c.g1, one_g2=BLS12_381_G2,
              x_g2=PA.g2_mul(BLS12_381_G2, x), z_g2=PA.g2_mul(BLS12_381_G2, z))
    TR = T.make_transcripts(c)
    assert PR.verify_proof(c, vk, proof, inst[1:], TR["merlin"], PA.pairing_check)
    bad = dict(proof, a_at_x1=(proof["a_at_x1"] + 1) % c.r)
    assert not PR.verify_proof(c, vk, bad, inst[1:], TR["merlin"], PA.pairing_check)


def test_prove_reference_bench_shape(gpu_ctx, oracle, api):
    """benches/bench.rs:38-61 shape at 2^11 - 100: unused witnesses (infinity bases in uj_wj_lcs),
    one repeated witness value, an empty last row."""
    from oracle.pyref.fields import BLS12_381 as c
    q, inst, wit = CI.bench_circuit(c, 1234567, 7654321, (1 << 11) - 100, (1 << 11) - 100)
    opk, gpk, _ = _prove_both(api, gpu_ctx, oracle, "bls12_381", q, inst, wit, 99)
    lcs = gpk.export_bases(5)
    assert (~lcs.any(axis=1)).sum() > 1000      # the unused-witness columns are points at infinity


def test_pk_load_path_equals_generate(gpu_ctx, oracle, api):
    """pm_pk_load of an existing key (arkworks 104-byte G1Affine stride) gives the same proof."""
    curve = "bls12_381"
    c = CURVES[curve]
    q, inst, wit = CI.synthetic_r1cs(c, 200)
    opk = oracle.OraclePk(curve, q, 1111, 2222, 4)
    arrays = []
    for i in range(6):
        b = opk.export_bases(i)
        wide = np.zeros((b.shape[0], 13), dtype=np.uint64)
        wide[:, :12] = b
        wide[:, 12] = (~b.any(axis=1)).astype(np.uint64)
        arrays.append(wide)
    A, B, C = pm_csrs(curve, q)
    gpk = api.ProvingKey.load(gpu_ctx, curve, opk.n, q.m0, q.mw, q.nr, opk.sigma, A, B, C, arrays)
    TR = T.make_transcripts(c)
    omega = oracle.fr_from_mont_limbs(curve, opk.omega_limbs)[0]
    po = DR.prove(opk, opk.n, opk.sigma, omega, inst, wit, [5, 6], TR["blake3"])
    pg = DR.prove(gpk, gpk.n, gpk.sigma, omega, inst, wit, [5, 6], TR["blake3"])
    assert po == pg


@pytest.mark.parametrize("curve", CURVE_LIST)
def test_setup_hook_sequence_generate_export_reload_proves_same_bytes(api, curve):
    """The sequence of the reference-side setup hook (rust/reference-patch: generator.rs:79 -> hip.rs: generate_bases_hip),
    through the same C ABI calls, at 2^16 - 100 gates: pm_pk_generate from the two trapdoor draws, pm_pk_info, the six
    vectors copied out in chunks with pm_pk_export_bases (GpuKey::export_bases: 2^18 points per call), rebuilt as arkworks'
    G1Affine records (104 / 72 bytes: x, y, `infinity: bool` -- the identity arrives as all-zero x, y), then a `prove` with
    (a) the key left resident by setup (GpuKeyCache::adopt) and (b) a second key made by pm_pk_load from the exported
    records (what a deserialised ProvingKey<E> goes through): the three transcripts' proof bytes must be identical."""
    from polymath_amd import circuits as PC
    from polymath_amd.polymath import Polymath
    c = CURVES[curve]
    nq = 6 if curve == "bls12_381" else 4
    nr = (1 << 16) - 100
    lc = PC.synthetic_r1cs_native(curve, nr)
    g = CI.SplitMix64(616)
    x, z, r_a = g.fr(c.r), g.fr(c.r), [g.fr(c.r), g.fr(c.r)]
    ctx_setup, ctx_prove = api.Context(0), api.Context(0)       # setup and prove may run on different threads' contexts
    pm = Polymath(curve, "merlin", ctx=ctx_setup)
    resident = pm.setup(lc, x, z)
    assert resident.n == 1 << 17 and resident.sigma == resident.n + 3 and resident.m0 == lc.m0
    lens = resident.base_lens
    n = resident.n
    # generator.rs:81-110 (max_index + 1 each); uj_wj_lcs: columns m0 .. 2 m0 + (m0 + mw) + nr of the SAP matrices (common.rs:130-134)
    assert list(lens) == [n + 1, 3, 2, 2 * (n - 1) + 8 * (n + 3) + 1, n - 1, 2 * lc.m0 + lc.mw + lc.nr]
    records = []
    for which in range(6):
        total, stride_words = int(lens[which]), 2 * nq + 1
        rec = np.zeros((total, stride_words), dtype=np.uint64)
        for off in range(0, total, 1 << 18):
            ln = min(1 << 18, total - off)
            xy = resident.export_bases(which, off, ln)
            rec[off:off + ln, :2 * nq] = xy
            rec[off:off + ln, 2 * nq] = (~xy.any(axis=1)).astype(np.uint64)      # Affine::identity(): infinity = true
        assert rec.strides[0] == (104 if curve == "bls12_381" else 72)
        records.append(rec)
    A, B, C = lc.csrs
    reloaded = api.ProvingKey.load(ctx_prove, curve, resident.n, lc.m0, lc.mw, lc.nr, resident.sigma, A, B, C, records)
    for tname in ("merlin", "keccak256", "blake3"):
        p_res = Polymath(curve, tname, ctx=ctx_prove).prove_native(resident.view(ctx_prove), lc.inst_limbs, lc.wit_limbs, r_a)
        p_rel = Polymath(curve, tname, ctx=ctx_prove).prove_native(reloaded, lc.inst_limbs, lc.wit_limbs, r_a)
        assert p_res == p_rel and len(p_res) == (176 if curve == "bls12_381" else 128)
    reloaded.free()
    resident.free()
    ctx_prove.close()
    ctx_setup.close()


def test_sharded_pk_partials_sum_to_whole(gpu_ctx, oracle, api):
    """MSM pairs sharded over ranks; partial points summed with pm_g1_sum equal the
    unsharded commitments (two shards emulated on one GPU)."""
    curve = "bls12_381"
    c = CURVES[curve]
    q, inst, wit = CI.synthetic_r1cs(c, 700)
    x = oracle.fr_to_mont_limbs(curve, inst)
    w = oracle.fr_to_mont_limbs(curve, wit)
    ra = oracle.fr_to_mont_limbs(curve, [31337, 271828])
    whole = _gpu_pk(api, gpu_ctx, curve, q, 4242, 2424, oracle)
    rc, a, ai, cc, ci = whole.phase1(x, w, ra)
    assert rc == 0
    x1, x2, av, cv = (oracle.fr_to_mont_limbs(curve, [v])[0] for v in (123456789, 987654321, 55, 66))
    parts_a, parts_c, parts_d = [], [], []
    ctx2 = api.Context(0)
    for rank in range(3):
        shard = _gpu_pk(api, ctx2, curve, q, 4242, 2424, oracle, shard_rank=rank, shard_count=3)
        rc, pa, pai, pc, pci = shard.phase1(x, w, ra)
        assert rc == 0
        parts_a.append(pa)
        parts_c.append(pc)
        # phase 3 with arbitrary challenges: the remainder check fails (not a real transcript),
        # so only compare when it passes -- use the real flow instead:
        shard.free()
    sa, _ = gpu_ctx.g1_sum(curve, np.stack(parts_a))
    sc_, _ = gpu_ctx.g1_sum(curve, np.stack(parts_c))
    assert np.array_equal(sa, a) and np.array_equal(sc_, cc)
    ctx2.close()


@pytest.mark.parametrize("shards", [4, 8])
def test_sharded_whole_proof_in_lockstep(gpu_ctx, oracle, api, shards):
    """The N-GPU data flow on one GPU: N shard keys (one context each, as N ranks would hold them) step through
    the three phases in lockstep, partial points are summed with pm_g1_sum exactly as PointCombiner does after
    the all-gather, and the proof bytes equal the unsharded key's."""
    from polymath_amd import circuits as PC
    from polymath_amd.polymath import Polymath
    curve = "bls12_381"
    r = CURVES[curve].r
    r1cs, inst, wit = PC.synthetic_r1cs(r, 5000)
    g = PC.SplitMix64(0x5AAD)
    x_t, z_t, r_a = g.fr(r), g.fr(r), [g.fr(r), g.fr(r)]
    whole = Polymath(curve, "keccak256", ctx=gpu_ctx)
    pk = whole.setup((r1cs, inst, wit), x_t, z_t)
    f = whole.field
    xl, wl = f.fr_limbs(inst), f.fr_limbs(wit)
    ref = whole.prove_limbs(pk, inst, xl, wl, r_a).to_bytes()
    pk.free()
    ranks = [Polymath(curve, "keccak256", device=0) for _ in range(shards)]
    pks = [pm.setup((r1cs, inst, wit), x_t, z_t, shard_rank=i, shard_count=shards) for i, pm in enumerate(ranks)]
    results = [None] * shards
    pending = {}          # round -> {rank: (partial point, infinity flag)}

    class _Yield(Exception):
        pass

    # cooperative lockstep without threads: replay each rank's prove_limbs until its next combine point
    def run_rank(i, answers):
        calls = {"n": 0}

        def combine(xy, inf):
            k = calls["n"]
            calls["n"] += 1
            if k < len(answers):
                return answers[k]
            pending.setdefault(k, {})[i] = (np.array(xy, dtype=np.uint64), inf)
            raise _Yield()
        return ranks[i].prove_limbs(pks[i], inst, xl, wl, r_a, combine)

    answers = []
    for rnd in range(3):                                    # [a], [c], [d]
        for i in range(shards):
            with pytest.raises(_Yield):
                run_rank(i, answers)
        pts = np.stack([pending[rnd][i][0] for i in range(shards)])
        infs = np.array([pending[rnd][i][1] for i in range(shards)], dtype=np.int32)
        answers.append(api.g1_sum(curve, pts, infs))
    for i in range(shards):
        results[i] = run_rank(i, answers).to_bytes()
    assert all(b == ref for b in results)
    for p in pks:
        p.free()


def test_native_whole_prove_equals_phase_by_phase(gpu_ctx):
    """pm_host_prove (C++ host glue inside the library: transcripts, challenge arithmetic, wire format) returns
    the fixture proofs byte for byte, for the three transcripts, host and device-resident assignment; an
    unsatisfied witness surfaces the phase status."""
    import ctypes as ct
    from polymath_amd import polymath as PM
    hip = ct.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ct.POINTER(ct.c_void_p), ct.c_size_t]
    hip.hipMemcpy.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_int]
    hip.hipFree.argtypes = [ct.c_void_p]
    for fx in load_golden("proofs.json"):
        q = r1cs_from_json(fx["r1cs"])
        inst, wit, r_a = [I(v) for v in fx["instance"]], [I(v) for v in fx["witness"]], [I(v) for v in fx["r_a"]]
        for tname, ref in fx["proofs"].items():
            pm = PM.Polymath("bls12_381", tname, ctx=gpu_ctx)
            pk = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), inst, wit), I(fx["x_trapdoor"]), I(fx["z_trapdoor"]))
            xl, wl = pm.field.fr_limbs(inst), pm.field.fr_limbs(wit)
            assert pm.prove_native(pk, xl, wl, r_a).hex() == ref["bytes"], (fx["name"], tname)
            if tname == "merlin":
                bufs = []
                for arr in (xl, wl):
                    p = ct.c_void_p()
                    assert hip.hipMalloc(ct.byref(p), max(arr.nbytes, 32)) == 0
                    assert hip.hipMemcpy(p, arr.ctypes.data_as(ct.c_void_p), arr.nbytes, 1) == 0
                    bufs.append(p)
                assert pm.prove_native(pk, xl, wl, r_a, device_ptrs=(bufs[0].value, bufs[1].value)).hex() == ref["bytes"]
                for p in bufs:
                    hip.hipFree(p)
                bad = list(wit)
                bad[0] = (bad[0] + 1) % pm.field.r
                with pytest.raises(PM.PolymathProverError) as e:
                    pm.prove_native(pk, xl, pm.field.fr_limbs(bad), r_a)
                assert e.value.status == 4                                    # PM_ERR_REMAINDER_NONZERO, prover.rs:108
            pk.free()


def test_error_codes(gpu_ctx, oracle, api):
    curve = "bls12_381"
    c = CURVES[curve]
    q, inst, wit = CI.synthetic_r1cs(c, 50)
    pk = _gpu_pk(api, gpu_ctx, curve, q, 77, 88, oracle)
    x, w = oracle.fr_to_mont_limbs(curve, inst), oracle.fr_to_mont_limbs(curve, wit)
    ra = oracle.fr_to_mont_limbs(curve, [1, 2])
    ctx3 = api.Context(0)
    pk3 = _gpu_pk(api, ctx3, curve, q, 77, 88, oracle)
    rc, _ = pk3.phase2(ra[0])
    assert rc == 8                                     # PM_ERR_STATE: phase 2 before phase 1
    bad = w.copy()
    bad[3] = oracle.fr_to_mont_limbs(curve, [12345])[0]
    rc = pk.phase1(x, bad, ra)[0]
    assert rc == 4                                     # PM_ERR_REMAINDER_NONZERO == prover.rs:108
    rc = pk.phase1(x, w, ra)[0]
    assert rc == 0
    one = oracle.fr_to_mont_limbs(curve, [1])[0]
    rc = pk.phase3(one, one, one, one)[0]
    assert rc == 4                                     # bogus challenge values: rem != 0, prover.rs:221
    bases = api.Bases.multiples(gpu_ctx, curve, 8)
    with pytest.raises(api.PolymathError) as e:
        bases.msm(rand_fr_limbs(curve, 9, 1))
    assert e.value.status == 2                         # scalars.len() > bases.len(), prover.rs:381
    pk3.free()
    ctx3.close()


def test_bench_two_ranks_one_gpu_same_proof():
    """bench.py's N > 1 flow end to end: 2 ranks (sharing the one GPU here, gloo instead of RCCL) each
    generate and hold half of every MSM pair range, all-gather partial points, and must print the same
    proof bytes as the single-rank run."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--full", "--steps", "1", "--warmup", "0", "--log-constraints", "12", "--no-cpu-baseline", "--msm-micro", "", "--no-live-traffic", "--other-configs", ""]
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + common, capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stderr[-3000:]
    env = dict(os.environ, BENCH_DIST_BACKEND="gloo", BENCH_FORCE_DEVICE="0")
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                          "127.0.0.1", "--master-port", "29544", os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                         capture_output=True, text=True, timeout=900, env=env)
    assert two.returncode == 0, two.stderr[-3000:]
    j1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    j2 = json.loads([l for l in two.stdout.splitlines() if l.startswith("{")][-1])
    assert j1["proof_bytes"] == j2["proof_bytes"] and j2["n_gpus"] == 2 and j2["scaling"] == "strong"
    assert "four-step NTT" in j2["config"]["parallelism"]          # the default N > 1 layout shards the vector phases too
    # ... and the pairs-only layout (vector phases replicated, points combined through torch.distributed) still agrees
    env["BENCH_SHARD_LAYOUT"] = "pairs"
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                          "127.0.0.1", "--master-port", "29545", os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                         capture_output=True, text=True, timeout=900, env=env)
    assert two.returncode == 0, two.stderr[-3000:]
    j3 = json.loads([l for l in two.stdout.splitlines() if l.startswith("{")][-1])
    assert j3["proof_bytes"] == j1["proof_bytes"] and "msm-pairs-sharded" in j3["config"]["parallelism"]


def test_bench_gpus_2_starts_its_own_ranks():
    """`python bench.py --gpus 2` with NO launcher (how the driver started round 2's bench): the parent spawns the two ranks
    itself (polymath_amd/launch.py; here sharing the one GPU over gloo), relays rank 0's line and exits 0; the line says two
    ranks were seen by the exchange layer and carries the single-GPU proof bytes.  `value` is the host-input metric
     and the HBM-resident variant is reported beside it."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--full", "--steps", "2", "--warmup", "1", "--log-constraints", "12", "--no-cpu-baseline", "--msm-micro", "", "--no-live-traffic", "--other-configs", ""]
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + common, capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stderr[-3000:]
    env = dict(os.environ, BENCH_DIST_BACKEND="gloo", BENCH_FORCE_DEVICE="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    two = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"] + common, capture_output=True, text=True, timeout=900, env=env)
    assert two.returncode == 0, two.stderr[-3000:]
    lines = [l for l in two.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    j2 = json.loads(lines[0])
    assert j2["n_gpus"] == 2 and j2["n_ranks_seen"] == 2 and j2["proof_bytes"] == j1["proof_bytes"] and j2["proof_verified"]
    assert j2["launch"]["supervised"] and "callbacks" in j2["exchange"]["kind"]
    for j in (j1, j2):
        assert abs(j["value"] - ((1 << 12) - 100) / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
        assert "HOST buffers" in j["timed_entry_point"] and j["ms_per_step_hbm_resident"] > 0


def test_bench_fallback_chain_when_rccl_cannot_serve_the_job():
    """Two ranks on ONE GPU with nothing pinned: RCCL refuses two ranks on one device, so attempt 0 (torch.distributed = nccl) dies
    in its first collective, the supervisor moves on, and the next attempt (gloo process group; the library's RCCL communicator
    fails to come up on every rank, so all of them agree on the host-staged exchange) completes.  What the launcher does on a
    fabric that will not come up, seen end to end: one JSON line, from a later attempt, with the single-GPU proof."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--full", "--steps", "2", "--warmup", "1", "--log-constraints", "12", "--no-cpu-baseline", "--msm-micro", "", "--no-live-traffic", "--other-configs", ""]
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + common, capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stderr[-3000:]
    env = dict(os.environ, BENCH_FORCE_DEVICE="0", BENCH_ATTEMPT_DEADLINE_S="300")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BENCH_DIST_BACKEND", "BENCH_NO_RCCL"):
        env.pop(k, None)
    two = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"] + common, capture_output=True, text=True, timeout=1500, env=env)
    assert two.returncode == 0, two.stderr[-3000:]
    lines = [l for l in two.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    j2 = json.loads(lines[0])
    assert j2["launch"]["attempt"] >= 1 and "attempt 0 failed" in two.stderr
    assert j2["n_gpus"] == 2 and j2["n_ranks_seen"] == 2 and j2["proof_bytes"] == j1["proof_bytes"] and j2["proof_verified"]
    assert j2["exchange"]["fallback_reason"]                      # ... and the line says why the preferred exchange was not used
    # the same under an external launcher (how the driver starts N > 1): every torchrun worker supervises its own rank's child;
    # the retry meets on a TCP store of its own, next to the launcher's
    three = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                            "--master-port", "29561", os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                           capture_output=True, text=True, timeout=1500, env=env)
    assert three.returncode == 0, three.stderr[-3000:]
    lines = [l for l in three.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j3 = json.loads(lines[0])
    assert j3["launch"]["attempt"] >= 1 and j3["n_ranks_seen"] == 2 and j3["proof_bytes"] == j1["proof_bytes"]


def test_bench_dead_rank_ends_the_job_non_zero():
    """A rank that dies in the middle of the timed proofs (test hook BENCH_TEST_DIE): the job exits NON-ZERO well inside the
    deadline -- no hang -- and prints no JSON line.  (Transport here: gloo callbacks; the library-level deadline and abort
    are covered by tests/test_sharded_vector.py.)"""
    import os, subprocess, sys, time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--steps", "100000", "--warmup", "1", "--log-constraints", "12", "--no-cpu-baseline", "--msm-micro", "", "--no-live-traffic", "--other-configs", ""]
    env = dict(os.environ, BENCH_DIST_BACKEND="gloo", BENCH_FORCE_DEVICE="0", BENCH_TEST_DIE="1,3.0", BENCH_COMM_TIMEOUT_S="20")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    t0 = time.time()
    run = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"] + common, capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode != 0
    assert not [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert "exited with code 17" in run.stderr or "failed" in run.stderr, run.stderr[-2000:]
    assert time.time() - t0 < 400


def test_bench_plain_run_is_lean_and_dumps_the_last_proof(tmp_path):
    """A plain `bench.py` run (no --full): the headline keys with `steps` = --steps and `value` from `ms_per_step`, none of
    --full's legs; --dump-outputs writes the last timed step's proof (proof.npy one float32 per byte, proof_bits.npy one per
    bit, LSB first), and a second run with the same arguments writes the same arrays."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for k in range(2):
        d = tmp_path / ("out%d" % k)
        run = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--log-constraints", "12",
                              "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stderr[-3000:]
        lines = [l for l in run.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        j = json.loads(lines[0])
        assert j["metric"] == "prove_constraints_per_sec" and j["unit"] == "constraints/s" and j["higher_is_better"] is True and j["dtype"] == "u32"
        assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0
        assert abs(j["value"] - ((1 << 12) - 100) / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
        for extra in ("ms_per_step_hbm_resident", "roofline", "valu", "stages", "proof_verified", "throughput_in_flight", "cpu_baseline",
                      "ntt_micro", "msm_micro", "other_configs"):
            assert extra not in j, extra
        proof, bits = np.load(d / "proof.npy"), np.load(d / "proof_bits.npy")
        assert proof.dtype == np.float32 and bits.dtype == np.float32
        raw = bytes.fromhex(j["proof_bytes"])
        assert len(raw) == 3 * 48 + 32 and proof.astype(np.uint8).tobytes() == raw
        assert np.array_equal(bits, np.unpackbits(np.frombuffer(raw, dtype=np.uint8), bitorder="little").astype(np.float32))
        dumps.append((proof, bits))
    assert all(np.array_equal(a, b) for a, b in zip(*dumps))


def test_full_size_2p20_proof_passes_pairing_verifier(oracle):
    """BASELINE configs[1] at full size: 2^20-100 synthetic gates (n = 2^21, 29.4 M MSM pairs).  The CPU
    restatement needs minutes here, so the check is the reference's own acceptance criterion
    (tests/mimc.rs:214): the pairing verifier (verifier.rs:19-62, oracle/pyref) accepts the GPU proof
    and rejects a tampered one; plus phase-1 outputs are on the curve."""
    from oracle.pyref import pairing as PA, protocol as PR
    from oracle.pyref.fields import BLS12_381 as c, BLS12_381_G2, g1_is_on_curve
    from polymath_amd import circuits as PC
    from polymath_amd.polymath import Polymath
    nr = (1 << 20) - 100
    r1cs, inst, wit = PC.synthetic_r1cs(c.r, nr)
    g = PC.SplitMix64(0xF00D)
    x, z, r_a = g.fr(c.r), g.fr(c.r), [g.fr(c.r), g.fr(c.r)]
    pm = Polymath("bls12_381", "merlin", device=0)
    pk = pm.setup((r1cs, inst, wit), x, z)
    assert pk.n == 1 << 21
    proof = pm.prove(pk, (r1cs, inst, wit), r_a).as_dict()
    assert all(g1_is_on_curve(c, proof[k]) for k in ("a_g1", "c_g1", "d_g1"))
    vk = dict(n=pk.n, m0=2, sigma=pk.sigma, omega=pk.omega, one_g1=c.g1, one_g2=BLS12_381_G2,
              x_g2=PA.g2_mul(BLS12_381_G2, x), z_g2=PA.g2_mul(BLS12_381_G2, z))
    TR = T.make_transcripts(c)
    assert PR.verify_proof(c, vk, proof, inst[1:], TR["merlin"], PA.pairing_check)
    bad = dict(proof, a_at_x1=(proof["a_at_x1"] + 1) % c.r)
    assert not PR.verify_proof(c, vk, bad, inst[1:], TR["merlin"], PA.pairing_check)
    # unsatisfied witness at full size -> PM_ERR_REMAINDER_NONZERO (prover.rs:108)
    from polymath_amd.polymath import PolymathProverError
    wit2 = list(wit)
    wit2[12345] = (wit2[12345] + 1) % c.r
    with pytest.raises(PolymathProverError) as e:
        pm.prove(pk, (r1cs, inst, wit2), r_a)
    assert (e.value.phase, e.value.status) == (1, 4)
    pk.free()


def test_reference_bench_circuit_skew(oracle):
    """benches/bench.rs:38-61 at 2^18 - 100 constraints: every padding witness carries the same value, so one
    bucket per window of the [c] MSM owns ~2^18 entries (SURVEY.md §8d "skewed worst case").  The pairing
    verifier accepts the proof; the hot buckets go through k_task_fold (a sequential sum took 268 ms at 2^20)."""
    import time
    from oracle.pyref import pairing as PA, protocol as PR
    from oracle.pyref.fields import BLS12_381 as c, BLS12_381_G2
    from polymath_amd import circuits as PC
    from polymath_amd.polymath import Polymath
    nc = (1 << 18) - 100
    g = PC.SplitMix64(0xBEAC4)
    pm = Polymath("bls12_381", "merlin", device=0)
    r1cs, inst, wit = pm._synthesize(PC.BenchCircuit(g.fr(c.r), g.fr(c.r), nc, nc))
    assert len(set(wit[2:])) == 1                                    # the skew itself
    x, z, r_a = g.fr(c.r), g.fr(c.r), [g.fr(c.r), g.fr(c.r)]
    pk = pm.setup((r1cs, inst, wit), x, z)
    xl, wl = pm.field.fr_limbs(inst), pm.field.fr_limbs(wit)
    pm.prove_limbs(pk, inst, xl, wl, r_a)
    t0 = time.perf_counter()
    proof = pm.prove_limbs(pk, inst, xl, wl, r_a)
    dt = time.perf_counter() - t0
    vk = dict(n=pk.n, m0=r1cs.m0, sigma=pk.sigma, omega=pk.omega, one_g1=c.g1, one_g2=BLS12_381_G2,
              x_g2=PA.g2_mul(BLS12_381_G2, x), z_g2=PA.g2_mul(BLS12_381_G2, z))
    assert PR.verify_proof(c, vk, proof.as_dict(), inst[1:], T.make_transcripts(c)["merlin"], PA.pairing_check)
    assert dt < 0.2, "skewed proof took %.0f ms: hot buckets are being reduced sequentially again" % (dt * 1e3)
    pk.free()
    # the same skew through the WIDE mode (no tables, one bucket set per window: the hot bucket of every window is folded inside
    # its own set) and through the per-window pipeline: identical bytes
    for mode in ("wide", "off"):
        pm.ctx.set_option("tables", mode)                  # the test's own context
        pk2 = pm.setup((r1cs, inst, wit), x, z)
        assert not pk2.msm_plan(1)[3]
        assert pm.prove_limbs(pk2, inst, xl, wl, r_a).to_bytes() == proof.to_bytes(), mode
        pk2.free()


def test_phase1_device_resident_assignment_equals_host(gpu_ctx, oracle, api):
    """pm_prove_phase1_device (assignment already in HBM) == pm_prove_phase1 (host buffers).  Device buffers
    come straight from the HIP runtime the library itself uses (no torch in this process)."""
    import ctypes as ct
    hip = ct.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ct.POINTER(ct.c_void_p), ct.c_size_t]
    hip.hipMemcpy.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_int]
    hip.hipFree.argtypes = [ct.c_void_p]

    def to_device(arr):
        p = ct.c_void_p()
        assert hip.hipMalloc(ct.byref(p), arr.nbytes) == 0
        assert hip.hipMemcpy(p, arr.ctypes.data_as(ct.c_void_p), arr.nbytes, 1) == 0   # hipMemcpyHostToDevice
        return p

    curve = "bls12_381"
    c = CURVES[curve]
    q, inst, wit = CI.synthetic_r1cs(c, 300)
    pk = _gpu_pk(api, gpu_ctx, curve, q, 1357, 2468, oracle)
    x, w = oracle.fr_to_mont_limbs(curve, inst), oracle.fr_to_mont_limbs(curve, wit)
    ra = oracle.fr_to_mont_limbs(curve, [11, 13])
    rc, a, ai, cc, ci = pk.phase1(x, w, ra)
    dx, dw = to_device(x), to_device(w)
    rc2, a2, ai2, cc2, ci2 = pk.phase1_device(dx.value, dw.value, ra)
    assert rc == rc2 == 0 and np.array_equal(a, a2) and np.array_equal(cc, cc2) and (ai, ci) == (ai2, ci2)
    hip.hipFree(dx)
    hip.hipFree(dw)


def test_setup_and_prove_with_the_reference_rng_signature(oracle):
    """Polymath.setup(circuit, rng) / .prove(pk, circuit, rng) -- the reference's own signatures (lib.rs:63-78) on its own random
    sources (polymath_amd/rng.py: StdRng = ChaCha12, seed_from_u64, Fp::rand, sample_element_outside_domain): the draws happen in
    the reference's order (generator.rs:72,77: x then z; prover.rs:110: r_a constant term first), so an independent replay of
    the stream feeds the CPU oracle the same values and the proofs are byte-identical.  benches/bench.rs:65 shape: seed 0."""
    from polymath_amd import circuits as PC, rng as R
    from polymath_amd.polymath import Polymath
    c = CURVES["bls12_381"]
    rng = R.StdRng.seed_from_u64(0)
    a, b = R.fr_rand(rng, c.r), R.fr_rand(rng, c.r)                  # bench.rs:67-68
    circuit = PC.BenchCircuit(a, b, 40, 37)
    pm = Polymath("bls12_381", "merlin", device=0)
    pk = pm.setup(circuit, rng)                                      # bench.rs:74
    proof = pm.prove(pk, circuit, rng)                               # bench.rs:79
    replay = R.StdRng.seed_from_u64(0)
    a2, b2 = R.fr_rand(replay, c.r), R.fr_rand(replay, c.r)
    x, z = R.sample_element_outside_domain(replay, c.r, pk.n), R.sample_element_outside_domain(replay, c.r, pk.n)
    r_a = [R.fr_rand(replay, c.r), R.fr_rand(replay, c.r)]
    assert (a2, b2) == (a, b) and pm.last_trapdoors == (x, z)
    q, inst, wit = CI.bench_circuit(c, a, b, 40, 37)
    opk = oracle.OraclePk("bls12_381", q, x, z, 2)
    omega = oracle.fr_from_mont_limbs("bls12_381", opk.omega_limbs)[0]
    ref = DR.prove(opk, opk.n, opk.sigma, omega, inst, wit, r_a, T.make_transcripts(c)["merlin"])
    assert proof.as_dict() == ref
    pk.free()


def test_device_field_products_match_host_cios(gpu_ctx):
    """pm_selftest_field: 2 x 4096 + edge products and squares per field on the device -- the dense reduced-radix product every
    kernel multiplies with (field.cuh: mul_r28, 9 x 29-bit limbs for the scalar fields) and the internal-radix product of the MSM /
    NTT inner loops (fq28.cuh) -- against the host's 32-bit CIOS, word for word.  (The arithmetic the reference takes from
    ark-ff, Cargo.toml:14; a compiler that drops a digit mask shows up here and not only as a wrong proof.)"""
    assert gpu_ctx.selftest_field(4096, seed=20260101) == {"bls12_381_fr": 0, "bn254_fr": 0, "bls12_381_fq": 0, "bn254_fq": 0}


@pytest.mark.parametrize("curve", CURVE_LIST)
@pytest.mark.parametrize("log_n", [11, 13, 14, 15, 16, 17, 18, 19, 20])
def test_ntt_extreme_inputs_vs_oracle(gpu_ctx, oracle, curve, log_n):
    """The reduced-radix tile kernels carry lazily (ntt.hip: values up to 37p, limbs up to 2^29 + 2^30 between carry
    propagations): inputs that push every butterfly to the top of its range -- all p - 1, p - 1 / 0 / 1 patterns, one spike --
    must still come out canonical and equal to the oracle's transform (prover.rs:241,319,325 call sites), both directions.
    11 = one 6- and one 5-stage pass, 13 = 7 + 6, 18 = two 9-stage passes, 19 = 7 + 6 + 6; 14 = 7 + 7 (a 7-stage pass in
    k_ntt_pass28, not only in the first-pass kernel), 15 = 8 + 7 and 16 = 8 + 8 (8-stage passes: values below 33p on the small
    tile, the `ns <= 7` argument of l28_emit false), 17 = 9 + 8, 20 = 7 + 7 + 6.
    What this does NOT tell apart is `ns <= 7` from `ns <= 8` in that argument: in the default build (PM_NTT_CANONICAL_QUOT = 1)
    both settings of short_pass reach f28_canonical_quot, whose code does not depend on JMAX, so the two branches are the same
    instructions.  They differ only in a PM_NTT_CANONICAL_QUOT = 0 build (conditional subtractions from 16p or from 32p)."""
    r = CURVES[curve].r
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    i = np.arange(n)
    pats = [                                   # (the distinct values, which of them every element takes)
        ([r - 1], np.zeros(n, dtype=np.int64)),
        ([0, r - 1], i & 1),
        ([1, r - 1], (i % 3 == 0).astype(np.int64)),
        ([r - 1, r - 2, r - 3, r - 4], rng.integers(0, 4, size=n)),
        ([0, r - 1], (i == n - 1).astype(np.int64)),
    ]
    for table, which in pats:
        a = oracle.fr_to_mont_limbs(curve, table)[which]
        for inverse in (False, True):
            assert np.array_equal(gpu_ctx.ntt(curve, a, log_n, inverse), oracle.ntt(curve, a, log_n, inverse, 8)), (log_n, inverse)


@pytest.mark.parametrize("curve", CURVE_LIST)
def test_msm_extreme_scalar_patterns(gpu_ctx, oracle, api, curve):
    """Scalars that sit on the signed-digit boundaries of every window layout (digit = 2^(c-1), 2^(c-1) + 1, all ones, carries
    rippling through every window, p - 1, (p +- 1) / 2, powers of two and their predecessors), on the per-window pipeline and
    on the window tables: the same point as the CPU oracle's MSM (prover.rs:380-384 call site)."""
    r = CURVES[curve].r
    pats = [r - 1, r - 2, (r - 1) // 2, (r + 1) // 2, 1, 2, 0]
    pats += [int("5" * 64, 16) % r, int("a" * 64, 16) % r, int("7f" * 32, 16) % r, int("80" * 32, 16) % r, int("f" * 63, 16) % r]
    for c in (15, 16, 20, 21, 22):                         # every digit exactly half / half + 1 for window width c
        pats += [sum(1 << (c * w + c - 1) for w in range(256 // c)) % r, sum((1 << (c - 1)) + 1 << (c * w) for w in range(256 // c)) % r]
    pats += [(1 << k) % r for k in range(0, 255, 7)] + [((1 << k) - 1) % r for k in range(1, 255, 7)]
    n = 4096
    vals = [pats[i % len(pats)] for i in range(n)]
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    hb = bases.download()
    sc = oracle.fr_to_mont_limbs(curve, vals)
    ref, rinf = oracle.msm(curve, hb, sc, 8)
    plain, inf = bases.msm(sc)
    assert inf == rinf and np.array_equal(plain, ref)
    bases.precompute()
    tabled, inf = bases.msm(sc)
    assert inf == rinf and np.array_equal(tabled, ref)


@pytest.mark.parametrize("curve", CURVE_LIST)
def test_msm_equal_bucket_sums_take_the_doubling_paths(gpu_ctx, oracle, api, curve, monkeypatch):
    """Every base the SAME point and scalars 1 .. NB used equally often: every bucket of the table path holds the same sum, so
    the reduction adds EQUAL points at every level -- the exceptional (doubling) branch of the one-lane additions of level 0 and
    of the four-lane cooperative additions of levels 1 / final (msm.hip: xyzz28_add_quad returns false on every lane of the
    quad, all four take the complete formulas).  Also with one scalar value only (all entries in one bucket: the hot-bucket
    fold).  Same point as the CPU oracle's MSM."""
    gpu_ctx.set_option("table_window_bits", 16)            # 2^15 buckets: the two-level reduction (>= 4096 buckets)
    n, nb = 1 << 17, 1 << 15
    g = oracle.g1_multiples(curve, 1)
    hb = np.repeat(g, n, axis=0)
    bases = api.Bases.upload(gpu_ctx, curve, hb)
    bases.precompute()
    for vals in ([(i % nb) + 1 for i in range(n)], [5] * n, [(i % 2) * (nb - 1) + 1 for i in range(n)]):
        sc = oracle.fr_to_mont_limbs(curve, vals)
        out, inf = bases.msm(sc)
        ref, rinf = oracle.msm(curve, hb, sc, 8)
        assert inf == rinf and np.array_equal(out, ref)
