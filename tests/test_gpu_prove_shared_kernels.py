"""GPU: the single prover and the batch prover launch one set of kernels (csrc/prove_kernels.cuh).  Shapes at which that shared text
takes a path no other batch test reaches, each proved by both provers on the same key and compared, row by row, with each other and
with the CPU oracle:

  m0 = 1, nr = 1 (n = 4):   the numerator has 63 coefficients: no chunked level, ONE lane divides with no carry-in array
  m0 = 1, nr = 3 (n = 8):   103 coefficients: one chunked level of 7 values under the one-lane top
  m0 = 9, nr = 7 (n = 32):  2 m0 = 18 > 16: the witness-only part of u is a zeroed head and a fifth transform, not the sparse sum

The rows of a batch share the circuit and the assignment (CI.random_r1cs gives one per circuit) and differ in r_a, so every
per-proof value -- r_a, x1, x2, the numerator's constants, the level multipliers -- differs from row to row.  A batch of one forwards
to the single prover.  One batch at n = 8 has a violated constraint in its middle row: that row alone is refused, with the single
prover's status.

Phase 1 between the uploads and the MSMs is one enqueue list for both provers (csrc/prove.hip: phase1_enqueue_u / phase1_enqueue_rest).
With msm_overlap = 0 the single prover takes the list's other branch -- no k_sc_a launch, k_phase1_scalars writes the [a]_1 scalars --
which no test above reaches; the batch prover's stays as it is.  Both must still give the oracle's bytes."""
import pytest

from oracle import driver as DR
from oracle.pyref import circuits as CI, serialize as SE, transcripts as T
from oracle.pyref.fields import CURVES

pytestmark = pytest.mark.gpu

PM_OK, PM_ERR_REMAINDER_NONZERO = 0, 4
_KEYS = {}


def _key(gpu_ctx, oracle, curve, m0, nr, n):
    """one GPU key, one oracle key, one satisfied assignment and three r_a per (curve, shape), shared by the tests"""
    from polymath_amd import polymath as PM
    k = (curve, m0, nr)
    if k not in _KEYS:
        c = CURVES[curve]
        q, inst, wit = CI.random_r1cs(c, 0x5A4E + 16 * m0 + nr, m0, nr)
        g = CI.SplitMix64(0x5A4E00 + 16 * m0 + nr)
        x, z = g.fr(c.r), g.fr(c.r)
        pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
        pk = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), inst, wit), x, z)
        assert (q.m0, q.nr, pk.n) == (m0, nr, n)
        opk = oracle.OraclePk(curve, q, x, z, 8)
        _KEYS[k] = dict(c=c, q=q, inst=inst, wit=wit, pm=pm, pk=pk, opk=opk, r_a=[[g.fr(c.r), g.fr(c.r)] for _ in range(3)],
                        xl=pm.field.fr_limbs(inst), wl=pm.field.fr_limbs(wit))
    return _KEYS[k]


def _oracle_bytes(s, oracle, curve):
    """the oracle's three proofs of a key (one per r_a), computed once"""
    if "want" not in s:
        opk, c = s["opk"], s["c"]
        omega = oracle.fr_from_mont_limbs(curve, opk.omega_limbs)[0]
        s["want"] = [SE.ser_proof(c, DR.prove(opk, opk.n, opk.sigma, omega, s["inst"], s["wit"], r_a, T.make_transcripts(c)["merlin"]))
                     for r_a in s["r_a"]]
    return s["want"]


@pytest.mark.parametrize("curve,m0,nr,n", [
    ("bls12_381", 1, 1, 4), ("bn254", 1, 1, 4),
    ("bls12_381", 1, 3, 8), ("bn254", 1, 3, 8),
    ("bls12_381", 9, 7, 32),
])
def test_small_shapes_bytes_equal_single_prover_and_oracle(gpu_ctx, oracle, curve, m0, nr, n):
    s = _key(gpu_ctx, oracle, curve, m0, nr, n)
    pm, pk = s["pm"], s["pk"]
    assert 8 * (n + 3) + 2 * n - 1 == {4: 63, 8: 103, 32: 343}[n]          # the numerator's length: <= 64 only at n = 4
    single = [pm.prove_native(pk, s["xl"], s["wl"], r_a) for r_a in s["r_a"]]
    want = _oracle_bytes(s, oracle, curve)
    assert len(set(single)) == 3
    for count in (1, 3):
        proofs, status = pm.prove_batch(pk, [(s["xl"], s["wl"])] * count, s["r_a"][:count])
        assert status == [PM_OK] * count, (count, status)
        for i in range(count):
            assert proofs[i] == single[i], (count, i, "single prover")
            assert proofs[i] == want[i], (count, i, "oracle")


@pytest.mark.parametrize("curve,m0,nr,n", [("bls12_381", 1, 1, 4), ("bn254", 1, 1, 4), ("bls12_381", 9, 7, 32)])
def test_msm_overlap_off_bytes_equal_oracle(gpu_ctx, oracle, curve, m0, nr, n):
    s = _key(gpu_ctx, oracle, curve, m0, nr, n)
    pm, pk = s["pm"], s["pk"]
    want = _oracle_bytes(s, oracle, curve)
    assert pm.ctx is gpu_ctx
    overlap_was = gpu_ctx.get_option("msm_overlap")
    gpu_ctx.set_option("msm_overlap", 0)
    try:
        single = [pm.prove_native(pk, s["xl"], s["wl"], r_a) for r_a in s["r_a"]]
        proofs, status = pm.prove_batch(pk, [(s["xl"], s["wl"])] * 3, s["r_a"])
    finally:
        gpu_ctx.set_option("msm_overlap", overlap_was)
    assert status == [PM_OK] * 3, status
    for i in range(3):
        assert single[i] == want[i], (i, "single prover")
        assert proofs[i] == want[i], (i, "batch prover")


def test_violated_row_in_the_middle_of_a_batch(gpu_ctx, oracle):
    from polymath_amd.polymath import PolymathProverError
    curve = "bls12_381"
    s = _key(gpu_ctx, oracle, curve, 1, 3, 8)
    pm, pk, q, c = s["pm"], s["pk"], s["q"], s["c"]
    bad = None
    for col in sorted({j for rows in (q.a, q.b, q.c) for row in rows for v, j in row if j >= q.m0 and v}):
        zz = list(s["inst"]) + list(s["wit"])
        zz[col] = (zz[col] + 1) % c.r
        if not all(CI.first_entry_dot(c.r, a, zz) * CI.first_entry_dot(c.r, b, zz) % c.r == CI.first_entry_dot(c.r, cc, zz)
                   for a, b, cc in zip(q.a, q.b, q.c)):
            bad = pm.field.fr_limbs(zz[q.m0:])
            break
    assert bad is not None
    with pytest.raises(PolymathProverError) as e:
        pm.prove_native(pk, s["xl"], bad, s["r_a"][1])
    assert e.value.status == PM_ERR_REMAINDER_NONZERO
    proofs, status = pm.prove_batch(pk, [(s["xl"], s["wl"]), (s["xl"], bad), (s["xl"], s["wl"])], s["r_a"])
    assert status == [PM_OK, PM_ERR_REMAINDER_NONZERO, PM_OK]
    assert proofs[1] is None
    for i in (0, 2):
        assert proofs[i] == pm.prove_native(pk, s["xl"], s["wl"], s["r_a"][i]), i
