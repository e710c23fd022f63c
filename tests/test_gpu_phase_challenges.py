"""GPU: pm_prove_phase2 / pm_prove_phase3 at HOSTILE challenge values, on the single prover and on the vector-sharded prover.

Every other test hands these two entry points values that came out of a hash.  The code behind them takes special paths at special
field elements -- x1^0 at x1 = 0 in the Horner lanes and the segment constants, level multipliers x1^(16^l) that collapse to 1, 0 or -1,
chains in reduced radix whose stored word must be 0 and not p when the value is an exact multiple of p, geometric tails with carry-in
times +-1 or 0 -- and the batch prover launches the same kernel text (csrc/prove_kernels.cuh).  The challenges come from
tests/phase_reference.py: challenge_grid (x1 in 0, +-1, +-2, 1/2, omega, 1/omega, omega^(n/2+1), a 2n-th root, an element of order 16,
one drawn value; x2 in 0, +-1, one drawn value, -1/(2 r_a[0])), on r_a sets with zeros, 1 and r - 1.

Per tuple: u(x1) equals the big-integer Horner sum and the oracle's; the status of phase 3 equals the reference's and the oracle's;
at status 0 [d]_1 equals the oracle's (pinned to the reference quotient by tests/test_phase_reference.py) and tap 7 equals the
reference quotient WORD FOR WORD -- a stored p where 0 belongs is the same residue and a different word.  A status-4 tuple always
follows a status-0 tuple of the same x1 and is followed by a status-0 tuple: a refused division must not poison the next one.  On the
single prover phase 3 takes its own x1, so phase 2 runs before the status-0 tuples only, the context still counts the earlier division
as done after a refusal, and tap 7 shows the REFUSED division's quotient: it is compared word for word too.  That is how the tuple
x1 = 0, x2 = (r - 1) / 2 on r_a = (1, 0) is seen at all: every coefficient of its u block is the lazy sum u_i + (p - u_i), its
remainder is x2 != 0, and its quotient words 5 sigma .. 5 sigma + n - 2 must be stored as 0.  The chains in reduced radix that this tuple
aims at (k_div_level0, k_div_expand0) are the single prover's; on the sharded prover phase 3 discards a refused division before tap 7
can be read, so there tap 7 is compared for the status-0 tuples only and a refused tuple is checked by its status on every rank.

Nothing is skipped at run time; the counts of status-0 tuples are asserted from the reference alone (phase_reference.check_grid_counts)."""
import numpy as np
import pytest

import phase_reference as REF
from helpers import fr_mont_limbs
from oracle.pyref.fields import CURVES
from test_gpu_prove_shared_kernels import _key
from test_sharded_vector import _oracle_reference, _run_ranks, _sharded_proofs

pytestmark = pytest.mark.gpu

PM_OK, PM_ERR_REMAINDER_NONZERO = 0, 4


def _expectations(oracle, curve, opk, xl, wl, r_a, x1_only=None, x2_only=None):
    """One oracle phase 1 with r_a, the grid for it, and per tuple (a generator): the tuple, u(x1) as limbs, the oracle's [d]_1 and the
    reference quotient as Montgomery limbs.  The oracle's u(x1) and status are asserted against the reference on the way.
    -> (number of tuples, generator)"""
    c, n, sigma = CURVES[curve], opk.n, opk.sigma
    omega = oracle.fr_from_mont_limbs(curve, opk.omega_limbs)[0]
    assert opk.phase1(xl, wl, fr_mont_limbs(curve, r_a))[0] == 0
    u, wit_u, u2 = REF.oracle_polys(oracle, curve, opk)
    grid, quots, nx1, nx2 = REF.challenge_grid(c, n, omega, r_a, sigma, u, wit_u, u2, x1_only, x2_only)
    n_ok = REF.check_grid_counts(grid, nx1, nx2)
    assert n_ok >= (nx1 - 1) * nx2 + 1
    for i in REF.lazy_tuple(c, grid, r_a):
        assert any(u) and not any(quots[i][5 * sigma:5 * sigma + n - 1])         # the lazy multiples of p occur

    def tuples():
        for t, q in zip(grid, quots):
            x1, x2, a_at, c_at, expect_rc = t
            L = [fr_mont_limbs(curve, [v]) for v in t[:4]]
            u_at = fr_mont_limbs(curve, [REF.horner(c, u, x1)])[0]
            rc, o_u_at = opk.phase2(L[0])
            assert rc == 0 and np.array_equal(o_u_at, u_at), t
            rc, d, d_inf = opk.phase3(*L)
            assert rc == expect_rc, t
            yield t, L, u_at, d, d_inf, fr_mont_limbs(curve, q)
    return len(grid), tuples()


def _first_difference(got, want):
    if got.shape != want.shape:
        return ("lengths", len(got), len(want))
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if len(bad) == 0 else ("quotient index", int(bad[0]), "of", len(want), got[bad[0]].tolist(), want[bad[0]].tolist())


def _single_grid(oracle, curve, s, r_a):
    """the grid for one r_a on the single prover's key s (test_gpu_prove_shared_kernels._key) -> tuples run"""
    pk, opk, n = s["pk"], s["opk"], s["pk"].n
    count, tuples = _expectations(oracle, curve, opk, s["xl"], s["wl"], r_a)
    assert pk.phase1(s["xl"], s["wl"], fr_mont_limbs(curve, r_a))[0] == PM_OK
    for w in (2, 5):                                                  # the vectors the reference was computed from are the GPU's
        assert np.array_equal(pk.tap(w, n), opk.tap(w, n)), w
    done, last = 0, None
    for t, L, u_at, d, d_inf, q in tuples:
        tag = (r_a, t)
        if t[4] == PM_OK:
            rc, got_u = pk.phase2(L[0])
            assert rc == PM_OK and np.array_equal(got_u, u_at), tag
        else:
            assert last is not None and last[4] == PM_OK and last[0] == t[0], tag      # tap 7 below reads the refused division
        rc, got_d, got_inf = pk.phase3(*L)
        assert rc == t[4], tag
        diff = _first_difference(pk.tap(7, 10 * n + 23), q)
        assert diff is None, (tag, diff)
        if rc == PM_OK:
            assert got_inf == d_inf and (d_inf or np.array_equal(got_d, d)), tag
        done, last = done + 1, t
    assert done == count
    return done


@pytest.mark.parametrize("curve,m0,nr,n", REF.SINGLE_SHAPES)
def test_single_prover_phases_on_the_hostile_grid(gpu_ctx, oracle, curve, m0, nr, n):
    """n = 4: 63 coefficients, the one-lane k_div_expand0 with a null carry-in.  n = 8: one chunked level of 7.  n = 32: the
    fifth-transform wit_u, one level of 22.  n = 128: two levels (82 -> 6), k_div_levelN and k_div_expandN once each.  n = 2048: three
    levels (20 503 coefficients -> 1282 -> 81 -> 6; sigma = n + 3 gives 8 sigma + 2n - 1 = 20 503), on r_a = (drawn, drawn) and (1, 0) with
    the full grid: 240 tuples whose expectations (a big-integer division and the oracle's MSM of 20 502 points on the CPU each) make
    this the slowest case of the file (7.7 s on the MI355X machine, 26 s of CPU work on eight slower cores); the grid is thinned only if
    the suite nears its time limit (profiles/phase_hostile_challenges.txt).  n = 8 runs r_a = (1, 0) once more with msm_overlap = 0 (k_phase1_scalars writes the [a]_1 scalars).
    At n = 32 and n = 128 phase 2 at every domain point returns the evaluation the transform started from (tap 0)."""
    c = CURVES[curve]
    r = c.r
    s = _key(gpu_ctx, oracle, curve, m0, nr, n)
    pk, sigma = s["pk"], s["pk"].sigma
    assert sigma == n + 3 and 8 * sigma + 2 * n - 1 == {4: 63, 8: 103, 32: 343, 128: 1303, 2048: 20503}[n]
    assert REF.level_plan(n, sigma) == {4: [], 8: [7], 32: [22], 128: [82, 6], 2048: [1282, 81, 6]}[n]
    for r_a in REF.single_r_a_sets(c, n):
        _single_grid(oracle, curve, s, r_a)
    if n == 8:
        overlap_was = gpu_ctx.get_option("msm_overlap")
        gpu_ctx.set_option("msm_overlap", 0)
        try:
            _single_grid(oracle, curve, s, [1, 0])
        finally:
            gpu_ctx.set_option("msm_overlap", overlap_was)
    if n in (32, 128):
        omega = oracle.fr_from_mont_limbs(curve, s["opk"].omega_limbs)[0]
        evals = pk.tap(0, n)
        assert len(evals) == n and np.array_equal(evals, s["opk"].tap(0, n))
        points = fr_mont_limbs(curve, [pow(omega, j, r) for j in range(n)])
        for j in range(n):
            rc, got = pk.phase2(points[j:j + 1])
            assert rc == PM_OK and np.array_equal(got, evals[j]), j


# ------------------------------------------------------------------------------------------------------ the sharded prover
_SHARDED = {}


def _sharded_case(oracle, curve, n, nr, sets_of, x1_only=None, x2_only=None):
    """circuit, trapdoors, the oracle's key and bytes, and per r_a set the list of _expectations' tuples: once per (curve, n)"""
    if (curve, n) not in _SHARDED:
        from polymath_amd import circuits as PC
        c = CURVES[curve]
        lc = PC.synthetic_r1cs_native(curve, nr)
        g = PC.SplitMix64(0x9A5D + n)
        x, z = g.fr(c.r), g.fr(c.r)
        sets = sets_of(REF.r_a_sets(c, n))
        want_bytes, opk = _oracle_reference(oracle, curve, lc, x, z, sets[0])
        assert opk.n == n
        x1_keep = None if x1_only is None else x1_only(c, oracle.fr_from_mont_limbs(curve, opk.omega_limbs)[0])
        x2_keep = None if x2_only is None else x2_only(c)
        per_set = []
        for r_a in sets:
            count, tuples = _expectations(oracle, curve, opk, lc.inst_limbs, lc.wit_limbs, r_a, x1_keep, x2_keep)
            per_set.append((r_a, list(tuples)))
            assert len(per_set[-1][1]) == count
        _SHARDED[(curve, n)] = dict(lc=lc, x=x, z=z, want_bytes=want_bytes, per_set=per_set)
    return _SHARDED[(curve, n)]


def _sharded_grid(curve, case, N, options):
    """N rank threads on one GPU: phase 1 per r_a set, then phase 2 and phase 3 per tuple (phase 3 of a sharded key needs the x1 of the
    phase 2 before it); every rank's answers against the expectations, the ranks' tap 7 scattered through their [d] pieces."""
    lc, n = case["lc"], None
    sets = [r_a for r_a, _ in case["per_set"]]
    pms, pks, comms, proofs = _sharded_proofs(curve, lc, case["x"], case["z"], sets[0], N, options=options)
    try:
        assert all(p == case["want_bytes"] for p in proofs)
        n = pks[0].n
        qn = 10 * n + 22
        off_ygz = min(p[0] for pk in pks for p in pk.msm_pieces(2))
        where = [np.concatenate([np.arange(lo - off_ygz, lo - off_ygz + cnt) for lo, cnt in pk.msm_pieces(2)]) for pk in pks]
        seen = np.bincount(np.concatenate(where), minlength=qn)
        assert len(seen) == qn and (seen == 1).all()                  # every quotient index on exactly one rank
        for r_a, tuples in case["per_set"]:
            ra_l = fr_mont_limbs(curve, r_a)

            def body(rk):
                pk, out = pks[rk], []
                assert pk.phase1(lc.inst_limbs, lc.wit_limbs, ra_l)[0] == PM_OK
                for t, L, u_at, d, d_inf, q in tuples:
                    rc2, got_u = pk.phase2(L[0])
                    rc3, got_d, got_inf = pk.phase3(*L)
                    out.append((rc2, got_u, rc3, got_d, got_inf, pk.tap(7, qn + 1) if rc3 == PM_OK else None))
                return out
            outs = _run_ranks(N, body, comms)
            for i, (t, L, u_at, d, d_inf, q) in enumerate(tuples):
                tag = (N, options, r_a, t)
                got = np.zeros((qn, 4), dtype=np.uint64)
                for rk in range(N):
                    rc2, got_u, rc3, got_d, got_inf, loc = outs[rk][i]
                    assert rc2 == PM_OK and np.array_equal(got_u, u_at), (tag, rk)
                    assert rc3 == t[4], (tag, rk)
                    if rc3 == PM_OK:
                        assert len(loc) == len(where[rk]), (tag, rk)
                        got[where[rk]] = loc
                if t[4] == PM_OK:
                    diff = _first_difference(got, q)
                    assert diff is None, (tag, diff)
                    for rk in range(N):
                        got_d, got_inf = outs[rk][i][3:5]
                        assert got_inf == d_inf and (d_inf or np.array_equal(got_d, d)), (tag, rk)
        assert not any(cm.failed for cm in comms)
        again = _run_ranks(N, lambda rk: pms[rk].prove_native(pks[rk], lc.inst_limbs, lc.wit_limbs, sets[0]), comms)
        assert all(p == case["want_bytes"] for p in again)
    finally:
        for pk in pks:
            pk.free()


@pytest.mark.parametrize("max_seg_log", [1, 3])
@pytest.mark.parametrize("n,nr,N", [(8, 2, 2), (32, 9, 2), (32, 9, 4)])
def test_sharded_prover_phases_on_the_hostile_grid(oracle, n, nr, N, max_seg_log):
    """bn254, sub-segments of 2 and 8 indices (every lane owns one index): the full grid on r_a = (drawn, drawn), (1, 0), (0, 0)"""
    case = _sharded_case(oracle, "bn254", n, nr, lambda sets: [sets[0], sets[2], sets[1]])
    _sharded_grid("bn254", case, N, {"max_seg_log": max_seg_log})


def test_sharded_prover_lanes_of_several_indices_on_the_hostile_grid(oracle):
    """n = 4096 (2046 gates), 2 ranks, bls12_381, the default sub-segment size: data blocks of 1024 indices and fillers of thousands, so
    a lane of k_seg_base / k_seg_expand owns 2 or more indices and seg_consts runs with pos - a > 0 INSIDE a lane's span, at hostile x1:
    index 2 sigma lies strictly inside a lane's span of its filler segment.  5 sigma is the first index of a block of the u region on
    every layout, hence always a lane's first index: it cannot be placed inside.  x1 in {0, 1, r - 1, omega, omega^(n/16), drawn},
    x2 in {0, r - 1, drawn}, r_a = (drawn, drawn)."""
    n, N = 4096, 2
    data_span, filler_span, off2, off5 = REF.sharded_geometry(n, N)
    assert data_span >= 2 and filler_span >= 2 and off2 > 0 and off5 == 0

    case = _sharded_case(oracle, "bls12_381", n, 2046, lambda sets: [sets[0]], lambda c, omega: REF.large_x1_only(c, n, omega),
                         lambda c: REF.large_x2_only(c, n))
    assert len({t[0][0] for t in case["per_set"][0][1]}) == 6 and len({t[0][1] for t in case["per_set"][0][1]}) == 3
    _sharded_grid("bls12_381", case, N, None)
