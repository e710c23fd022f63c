"""Phases 2 and 3 of the prover on plain Python integers (test infrastructure): the numerator of prover.rs:211-216, its division by
(X - x1) and u(x1), written from the dense transcription oracle/pyref/protocol.py:361-386 -- no limbs, no oracle/cpp, no kernel text --
and the grid of HOSTILE challenges that tests/test_phase_reference.py (CPU: the C++ oracle against this file) and
tests/test_gpu_phase_challenges.py (both GPU provers against this file and the oracle) feed to pm_prove_phase2 / pm_prove_phase3.

Everything is exact arithmetic mod r.  The first argument of every function is the curve object (oracle.pyref.fields.CURVES[...])."""
from oracle.pyref import protocol as PR

MINUS_ALPHA, MINUS_GAMMA = PR.MINUS_ALPHA, PR.MINUS_GAMMA     # 3 and 5: the numerator is the reference's times X^(5 sigma)
PM_OK, PM_ERR_REMAINDER_NONZERO = 0, 4


class SplitMix64:
    """the generator of oracle/pyref/circuits.py, restated so that this file draws its own values"""

    def __init__(self, seed):
        self.s = seed & (2 ** 64 - 1)

    def next_u64(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return z ^ (z >> 31)

    def fr(self, r):
        v = 0
        for _ in range(5):
            v = (v << 64) | self.next_u64()
        return v % r


def square(c, u):
    """u^2 as 2 len(u) - 1 coefficients (not stripped): schoolbook up to 128 coefficients, pyref's transform above that
    (square_polynomial, prover.rs:315-328)"""
    r, n = c.r, len(u)
    if n <= 128:
        out = [0] * (2 * n - 1)
        for i, x in enumerate(u):
            if x:
                for j, y in enumerate(u):
                    out[i + j] = (out[i + j] + x * y) % r
        return out
    n2 = PR.next_pow2(2 * n)
    ev = PR.ntt_fast(c, u, n2)
    out = PR.ntt_fast(c, [e * e % r for e in ev], n2, inverse=True)
    assert not any(out[2 * n - 1:])
    return out[:2 * n - 1]


def numerator(c, n, sigma, u, wit_u, u2, r_a, x2, a_at, c_at):
    """The 8 sigma + 2n - 1 coefficients of prover.rs:211-216 times X^(5 sigma) (protocol.py:361-379, term by term):
        a_by = u X^(5s) + r_a X^(2s)                                              :145-152
        r_by = 2 r_a u X^(5s) + r_a^2 X^(2s) + r_a                                :359-377
        c_by = wit_u X^(3s) + (wit_w + h_num) X^(8s) + r_by,  wit_w + h_num = u^2 :168-185 (the W witness part is w itself)
        num  = a_by + x2 c_by - (a_at + x2 c_at) X^(5s)                           :211-216"""
    r, s = c.r, sigma
    assert len(u) == n and len(wit_u) == n and len(u2) == 2 * n - 1 and len(r_a) == 2
    a_by = [0] * (8 * s + 2 * n - 1)
    c_by = [0] * (8 * s + 2 * n - 1)
    a_by[MINUS_GAMMA * s:MINUS_GAMMA * s + n] = u
    a_by[(MINUS_GAMMA - MINUS_ALPHA) * s:(MINUS_GAMMA - MINUS_ALPHA) * s + 2] = r_a
    two_ra_u = [2 * (r_a[0] * hi + r_a[1] * lo) % r for lo, hi in zip([0] + list(u), list(u) + [0])]      # 2 r_a u: n + 1 words
    ra_sq = [r_a[0] * r_a[0] % r, 2 * r_a[0] * r_a[1] % r, r_a[1] * r_a[1] % r]
    c_by[MINUS_GAMMA * s:MINUS_GAMMA * s + n + 1] = two_ra_u
    c_by[(MINUS_GAMMA - MINUS_ALPHA) * s:(MINUS_GAMMA - MINUS_ALPHA) * s + 3] = ra_sq
    c_by[0:2] = r_a
    c_by[MINUS_ALPHA * s:MINUS_ALPHA * s + n] = wit_u
    c_by[(MINUS_ALPHA + MINUS_GAMMA) * s:] = u2
    assert len(a_by) == len(c_by) == 8 * s + 2 * n - 1               # the blocks do not overlap: every slice kept its length
    num = [(a + x2 * b) % r if b else a for a, b in zip(a_by, c_by)]
    num[MINUS_GAMMA * s] = (num[MINUS_GAMMA * s] - a_at - c_at * x2) % r
    return num


def divide(c, num, x1):
    """(quotient, remainder) of num by (X - x1): the serial recurrence of protocol.py:381-386; the quotient keeps its len(num) - 1 words"""
    r = c.r
    q = [0] * (len(num) - 1)
    carry = 0
    for k in range(len(num) - 1, 0, -1):
        carry = (num[k] + x1 * carry) % r
        q[k - 1] = carry
    return q, (num[0] + x1 * carry) % r


def horner(c, u, x1):
    acc = 0
    for coef in reversed(u):
        acc = (acc * x1 + coef) % c.r
    return acc


def solve_a_at(c, n, sigma, u, wit_u, u2, r_a, x1, x2, c_at):
    """x1 != 0: the a_at with remainder zero for this c_at.  a_at enters the numerator once, with coefficient -1 at 5 sigma, so
    0 = N(x1) = N'(x1) - (a_at + x2 c_at) x1^(5 sigma) with N' the numerator for a_at = c_at = 0:  a_at = S - x2 c_at,
    S = sum_k N'_k x1^(k - 5 sigma)."""
    r = c.r
    assert x1 % r
    return _solve(c, sigma, numerator(c, n, sigma, u, wit_u, u2, r_a, x2, 0, 0), x1, x2, c_at)


def _solve(c, sigma, bare, x1, x2, c_at):
    S = horner(c, bare, x1) * pow(x1, -MINUS_GAMMA * sigma, c.r) % c.r
    return (S - x2 * c_at) % c.r


def x1_values(c, n, omega):
    """the hostile first challenges, in a fixed order without repeats: 0 first"""
    r = c.r
    psi = c.root_of_unity(2 * n)
    assert pow(psi, n, r) == r - 1 and pow(omega, n, r) == 1 and pow(omega, n // 2, r) == r - 1
    vals = [0, 1, r - 1, 2, r - 2, pow(2, -1, r), omega, pow(omega, -1, r), pow(omega, n // 2 + 1, r), psi]
    if n >= 16:
        w16 = pow(omega, n // 16, r)
        assert pow(w16, 16, r) == 1 and pow(w16, 8, r) != 1          # order 16: x1^16 = 1, every level multiplier of the scan is 1
        vals.append(w16)
    vals.append(SplitMix64(0x9051 + n).fr(r))
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    return out


def x2_values(c, n, r_a):
    r = c.r
    vals = [0, 1, r - 1, SplitMix64(0x9052 + n).fr(r)]
    if r_a[0] % r:
        vals.append(-pow(2 * r_a[0], -1, r) % r)                      # 2 x2 r_a[0] = -1: with r_a[1] = 0 the u block of the numerator vanishes
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    return out


def challenge_grid(c, n, omega, r_a, sigma, u, wit_u, u2, x1_only=None, x2_only=None):
    """-> (tuples, quotients, |X1|, |X2|), tuples = [(x1, x2, a_at, c_at, expect_rc), ...], deterministic, grouped by x1;
    quotients[i] is divide()'s quotient of tuple i (the division that gave expect_rc: computed once, handed on).

    x1 != 0: for every x2 one tuple with a_at = solve_a_at (status 0), then the same with a_at + 1 (status 4).
    x1 == 0: the remainder is N_0 = x2 r_a[0] whatever a_at and c_at are: status 4 unless that product is 0.  Every status-4 tuple there
    is FOLLOWED by a status-0 tuple (x2 = 0, fresh a_at and c_at), and the group starts with one; the last status-0 tuple is repeated
    at the end.  So in the whole grid a status-4 tuple has a status-0 tuple of the same x1 before it and a status-0 tuple after it.
    c_at cycles through 0, 1, r - 1 and a drawn value.  expect_rc comes from divide() on the reference numerator and is asserted
    against the rule.  x1_only / x2_only: predicates that thin the two lists (the largest shapes)."""
    r = c.r
    g = SplitMix64(0x9053 + n)
    c_cycle = [0, 1, r - 1, g.fr(r)]
    X1 = [v for v in x1_values(c, n, omega) if x1_only is None or x1_only(v)]
    X2 = [v for v in x2_values(c, n, r_a) if x2_only is None or x2_only(v)]
    assert X1[0] == 0 and X2[0] == 0
    out, quots, turn = [], [], 0

    def emit(x1, x2, a_at, c_at, rule, bare=None):
        num = list(bare) if bare else numerator(c, n, sigma, u, wit_u, u2, r_a, x2, a_at, c_at)
        if bare:                                                      # the numerator for a_at = c_at = 0, already at hand
            num[MINUS_GAMMA * sigma] = (num[MINUS_GAMMA * sigma] - a_at - c_at * x2) % r
        q, rem = divide(c, num, x1)
        rc = PM_OK if rem == 0 else PM_ERR_REMAINDER_NONZERO
        assert rc == rule, (x1, x2, a_at, c_at, rc, rule)
        out.append((x1, x2, a_at, c_at, rc))
        quots.append(q)

    for x1 in X1:
        for x2 in X2:
            c_at = c_cycle[turn % 4]
            turn += 1
            if x1 == 0:
                a_at = g.fr(r)
                if x2 * r_a[0] % r == 0:
                    emit(0, x2, a_at, c_at, PM_OK)
                else:
                    emit(0, x2, a_at, c_at, PM_ERR_REMAINDER_NONZERO)
                    emit(0, 0, g.fr(r), c_cycle[turn % 4], PM_OK)
            else:
                bare = numerator(c, n, sigma, u, wit_u, u2, r_a, x2, 0, 0)
                a_at = _solve(c, sigma, bare, x1, x2, c_at)             # solve_a_at
                emit(x1, x2, a_at, c_at, PM_OK, bare)
                emit(x1, x2, (a_at + 1) % r, c_at, PM_ERR_REMAINDER_NONZERO, bare)
    out.append(out[-2])                                               # the grid ends on a status-0 tuple
    quots.append(quots[-2])
    return out, quots, len(X1), len(X2)


def check_grid_counts(grid, nx1, nx2):
    """the conditions every test asserts on its grid, from the reference alone: at least (|X1| - 1) |X2| status-0 tuples with
    x1 != 0, one status-0 tuple with x1 = 0, every status-4 tuple between two status-0 tuples"""
    ok = [t for t in grid if t[4] == PM_OK]
    assert sum(1 for t in ok if t[0] != 0) >= (nx1 - 1) * nx2 > 0
    assert any(t[0] == 0 for t in ok)
    assert grid[0][4] == PM_OK and grid[-1][4] == PM_OK
    for i, t in enumerate(grid):
        if t[4] != PM_OK:
            assert grid[i - 1][4] == PM_OK and grid[i - 1][0] == t[0] and grid[i + 1][4] == PM_OK, i
    return len(ok)


def r_a_sets(c, seed):
    """(rand, rand), (0, 0), (1, 0), (r - 1, r - 1), (0, 1)"""
    g = SplitMix64(0x9054 + seed)
    return [[g.fr(c.r), g.fr(c.r)], [0, 0], [1, 0], [c.r - 1, c.r - 1], [0, 1]]


SINGLE_SHAPES = [("bls12_381", 1, 1, 4), ("bn254", 1, 1, 4), ("bls12_381", 1, 3, 8), ("bn254", 1, 3, 8), ("bls12_381", 9, 7, 32),
                 ("bn254", 2, 62, 128), ("bls12_381", 2, 1022, 2048)]      # (curve, m0, nr, n) of the single prover's tests


def single_r_a_sets(c, n):
    """the r_a sets of the single prover's test at size n: all five, at n = 2048 (drawn, drawn) and (1, 0)"""
    sets = r_a_sets(c, n)
    return [sets[0], sets[2]] if n == 2048 else sets


def large_x1_only(c, n, omega):
    """the sharded n = 4096 test keeps x1 in {0, 1, r - 1, omega, omega^(n/16), drawn}"""
    keep = (0, 1, c.r - 1, omega, pow(omega, n // 16, c.r), x1_values(c, n, omega)[-1])
    return lambda v: v in keep


def large_x2_only(c, n):
    """... and x2 in {0, r - 1, drawn}"""
    keep = (0, c.r - 1, x2_values(c, n, [0, 0])[3])
    return lambda v: v in keep


def level_plan(n, sigma):
    """the level counts of the single prover's division scan above the numerator: the arithmetic of proof_shape (csrc/prove_common.cuh)"""
    cnt, plan = 8 * sigma + 2 * n - 1, []
    while cnt > 64 and len(plan) < 6:
        cnt = (cnt + 15) // 16
        plan.append(cnt)
    return plan


def oracle_polys(oracle, curve, opk):
    """u, wit_u (taps 2 and 5 of the proof in flight on the oracle's key, as integers, n words each) and u^2"""
    from oracle.pyref.fields import CURVES
    c, n = CURVES[curve], opk.n
    u = oracle.fr_from_mont_limbs(curve, opk.tap(2, n))
    wit_u = oracle.fr_from_mont_limbs(curve, opk.tap(5, n))
    u, wit_u = u + [0] * (n - len(u)), wit_u + [0] * (n - len(wit_u))
    return u, wit_u, square(c, u)


def lazy_tuple(c, grid, r_a):
    """the tuples x1 = 0, x2 = (r - 1) / 2 of a grid; on r_a = (1, 0) there is exactly one and its status is 4 (remainder x2)"""
    found = [i for i, t in enumerate(grid) if t[0] == 0 and t[1] == (c.r - 1) // 2]
    if list(r_a) == [1, 0]:
        assert len(found) == 1 and grid[found[0]][4] == PM_ERR_REMAINDER_NONZERO
    return found


def lane_spans(starts, total, lanes=512):
    """[(a, b, span)] for the sub-segments cut at `starts`: a lane of the segment owns `span` consecutive indices
    (csrc/prove_sharded.hip: k_seg_base, k_seg_expand)"""
    cuts = sorted(starts) + [total]
    return [(a, b, (b - a + lanes - 1) // lanes) for a, b in zip(cuts, cuts[1:])]


def default_max_seg(n, N):
    """pick_max_seg of polymath_amd/host/layout.hpp"""
    ms = 1 << 13
    while (10 * n + 23) // N // ms > 384:
        ms <<= 1
    return ms


def sharded_geometry(n, N):
    """-> (longest data span, longest filler span, offset of 2 sigma inside its lane, offset of 5 sigma inside its lane)"""
    from test_sharded_vector import _segment_starts
    s = n + 3
    segs = lane_spans(_segment_starts(n, N, default_max_seg(n, N)), 10 * n + 23)
    data = lambda a: 3 * s <= a < 3 * s + n or 5 * s <= a <= 5 * s + n or a >= 8 * s
    inside = lambda k: [(k - a) % span for a, b, span in segs if a <= k < b][0]
    return (max(span for a, b, span in segs if data(a)), max(span for a, b, span in segs if not data(a)), inside(2 * s), inside(5 * s))
