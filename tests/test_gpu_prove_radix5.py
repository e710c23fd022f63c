"""GPU: whole proofs whose three MSMs run on window tables of radix 5*2^a (csrc/radix.cuh), and on the power-of-two layout forced
through the same developer option, bit-exact against oracle/cpp: 2^12 - 100 and 2^16 - 100 gates on BLS12-381, 2^12 - 100 on BN254.

table_window_bits = 100 m + windows (read by pm_pk_generate).  511: 11 windows of radix 5*2^21, 5.24 M buckets in 160 sort regions,
level-0 fan-in K0 = 40 and level 1's double-and-add over K0's bits; 512: 12 windows of 5*2^19, 1.31 M buckets in 40 regions, K0 = 10 --
the two plans the cost model picks for long MSMs; 514: 5 regions, K0 = 4; 112: today's 12 windows of 22 / 21 bits."""
import os

import numpy as np
import pytest

from oracle import driver as DR
from oracle.pyref import circuits as CI, serialize as SE, transcripts as T
from oracle.pyref.fields import CURVES

pytestmark = pytest.mark.gpu

_ORACLE = {}       # (curve, log_nr) -> the oracle's proof and the bases it proved on

CASES = [("bls12_381", 12, 514), ("bls12_381", 12, 511), ("bls12_381", 12, 112),
         ("bls12_381", 16, 511), ("bls12_381", 16, 512), ("bls12_381", 16, 112),
         ("bn254", 12, 514), ("bn254", 12, 512), ("bn254", 12, 112)]


@pytest.mark.parametrize("curve,log_nr,force", CASES, ids=["%s-%d-%d" % c for c in CASES])
def test_proof_on_forced_radix_vs_oracle(gpu_ctx, oracle, curve, log_nr, force):
    from polymath_amd import circuits as PC
    from polymath_amd.polymath import Polymath
    gpu_ctx.set_option("table_window_bits", force)              # restored by conftest
    c = CURVES[curve]
    nr = (1 << log_nr) - 100
    q, inst, wit = CI.synthetic_r1cs(c, nr)
    g = CI.SplitMix64(5500 + log_nr)
    x, z, r_a = g.fr(c.r), g.fr(c.r), [g.fr(c.r), g.fr(c.r)]
    lc = PC.synthetic_r1cs_native(curve, nr)
    pm = Polymath(curve, "merlin", ctx=gpu_ctx)
    gpk = pm.setup(lc, x, z)
    m, windows = divmod(force, 100)
    bits = {(5, 11): 24, (5, 12): 22, (5, 14): 19, (1, 12): 22}[(m, windows)]          # m = 5: ceil(log2 R) = a + 3
    assert all(gpk.msm_plan(k)[1:] == (windows, bits, True) for k in range(3)), [gpk.msm_plan(k) for k in range(3)]
    exported = [gpk.export_bases(i) for i in range(6)]
    memo = _ORACLE.get((curve, log_nr))
    if memo is None:                                            # once per (curve, size): the key's layout does not enter
        opk = oracle.OraclePk(curve, q, None, None, os.cpu_count() or 8)
        for i in range(6):
            opk.import_bases(i, exported[i])
        omega = oracle.fr_from_mont_limbs(curve, opk.omega_limbs)[0]
        po = DR.prove(opk, opk.n, opk.sigma, omega, inst, wit, r_a, T.make_transcripts(c)["merlin"])
        memo = {"omega": omega, "proof": po, "bases": [b.copy() for b in exported]}
        _ORACLE.clear()
        _ORACLE[(curve, log_nr)] = memo
    assert all(np.array_equal(a, b) for a, b in zip(exported, memo["bases"]))
    assert memo["omega"] == gpk.omega
    pg = DR.prove(gpk, gpk.n, gpk.sigma, memo["omega"], inst, wit, r_a, T.make_transcripts(c)["merlin"])
    assert pg == memo["proof"]
    assert pm.prove_native(gpk, lc.inst_limbs, lc.wit_limbs, r_a) == SE.ser_proof(c, memo["proof"])
    gpk.free()
