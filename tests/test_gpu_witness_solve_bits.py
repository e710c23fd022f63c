"""GPU: PM_ASSIGNMENT_SOLVE on boolean circuits -- booleanity rows and bit decompositions (csrc/solve.hip: solve_bits, k_solve_bits,
the decomposition branch of k_solve_chain; host/solve_plan.hpp with the modulus).  The bar is equality, word for word, with Python
integers: the generators' own assignments (polymath_amd.circuits: RangeCheck, ArxDemo / arx_native) and hand evaluation.

Shapes are the smallest at which each mechanism can differ.  RangeCheck with N values is ONE level of N decompositions: N = 1 and
31 are walked by the chain kernel, 32 is the first level with a k_solve_bits launch of its own, 64 is a whole wave of it, 257 a
256-lane workgroup and one lane; batches of 1, 3 and 70 are the chain kernel's partial wave and second workgroup and k_solve_bits'
grid y.  k = 254 / 253 is the widest decomposition either field allows (every limb of T is read); k + 1 is refused.  The hand-built
system has one decomposition of each kind beside ordinary steps; ArxDemo mixes decompositions in A and in C, XOR rows that solve
boolean-pending columns and recompositions, at width 8 over 2 rounds and at width 32 (every bit of a limb) over 1."""
import ctypes as ct

import numpy as np
import pytest
import torch        # noqa: F401  before libpolymath_hip.so is loaded: torch brings its own HIP runtime (tests/ntt_device_child.py)

from oracle.pyref.fields import CURVES
from witness_solve_helpers import BOTH, NONE, PM_ERR_INVALID_ARG, PM_OK, _setup, key_cache

pytestmark = pytest.mark.gpu

PROOF_LEN = {"bls12_381": 176, "bn254": 128}
_cached = key_cache()


def _stack(s, partials):
    pairs = [s["pm"].partial_limbs(i, w) for i, w in partials]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _full_limbs(s, inst, wit):
    return np.concatenate([s["f"].fr_limbs(inst), s["f"].fr_limbs(wit)])


def _solve_and_check(s, xs, ws, max_rows=2):
    """r1cs_check_batch(solve=True) on host limbs -> (n_bad, rows, stuck words, completed x || w rows)"""
    rc, n_bad, rows, _ = s["pk"].r1cs_check_batch(xs, ws, max_rows, solve=True)
    assert rc == PM_OK, s["pm"].ctx.last_error()
    stuck, _ = s["pk"].solve_results(len(xs))
    return [int(v) for v in n_bad], rows, [int(v) for v in stuck], s["pk"].solved_assignments(len(xs), s["q"].mw)


# ---- 1. RangeCheck: one level of N decompositions, at the chain / level threshold and the wave and workgroup edges of k_solve_bits ---------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("n_values", [1, 31, 32, 64, 257])
def test_range_check(gpu_ctx, curve, n_values):
    from polymath_amd import api, circuits as PC
    bits = 8
    s = _cached((curve, "range", n_values), lambda: _setup(gpu_ctx, curve, PC.RangeCheck([(3 + i) % 256 for i in range(n_values)], bits), 9100 + n_values))
    f, q = s["f"], s["q"]
    assert (q.m0, q.mw, q.nr) == (1, n_values * (1 + bits), n_values * (1 + bits))
    small = f.fr_limbs(list(range(1 << bits))).reshape(-1, 4)              # the limbs of 0 .. 255: every value of these assignments
    g = PC.SplitMix64(9200 + n_values)
    given = np.zeros(1 + q.mw, dtype=bool)
    given[0] = True
    given[1::1 + bits] = True                                               # column 0 and every v
    for count in (1, 3, 70):
        values = [[g.next_u64() % (1 << bits) for _ in range(n_values)] for _ in range(count)]
        values[0][0], values[-1][-1] = (1 << bits) - 1, 0                   # all bits set, no bit set
        want = np.stack([small[np.array([1] + PC.RangeCheck(v, bits).native())] for v in values])
        partial = want.copy()
        partial[:, ~given] = api.UNKNOWN_LIMBS
        n_bad, _, stuck, full = _solve_and_check(s, np.ascontiguousarray(partial[:, :1]), np.ascontiguousarray(partial[:, 1:]))
        assert n_bad == [0] * count and stuck == [NONE] * count, (count, n_bad, stuck)
        assert np.array_equal(full, want), count


# ---- 2. the widest decomposition: k = bitlength(r) - 1; one more bit is refused ------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_widest_decomposition(gpu_ctx, curve):
    from polymath_amd import api, circuits as PC
    c = CURVES[curve]
    k = c.r.bit_length() - 1
    assert k == {"bls12_381": 254, "bn254": 253}[curve]
    s = _cached((curve, "widest"), lambda: _setup(gpu_ctx, curve, PC.RangeCheck([5], k), 9300))
    pm, pk = s["pm"], s["pk"]
    values = [(1 << k) - 1, PC.SplitMix64(9301).fr(c.r) >> 1, 1 << (k - 1), 1]
    assert all(v < 1 << k for v in values)
    got = pm.solve_batch(pk, [pm.partial_limbs(*PC.RangeCheck([v], k).partial(c.r)) for v in values])
    assert got == [(None, [1], PC.RangeCheck([v], k).native()) for v in values]
    assert pm.check_batch(pk, [pm.partial_limbs(*PC.RangeCheck([v], k).partial(c.r)) for v in values[:2]], max_rows=2, solve=True) == [(0, [])] * 2
    # 2^k has no k-bit form (and is still a field element): stuck at the decomposition row, row k
    assert pm.solve_batch(pk, [pm.partial_limbs([1], [1 << k] + [None] * k)]) == [(k, None, None)]

    # k + 1 bits: the solution would not be unique.  PM_ERR_INVALID_ARG from every entry point, outputs untouched
    wide = _cached((curve, "too wide"), lambda: _setup(gpu_ctx, curve, PC.RangeCheck([5], k + 1), 9302))
    L, vp, h, plen, f = gpu_ctx.L, (lambda a: a.ctypes.data_as(ct.c_void_p)), wide["pk"].h, PROOF_LEN[curve], wide["f"]
    xs, ws = _stack(wide, [PC.RangeCheck([5], k + 1).partial(c.r)] * 3)
    text = "row %d" % (k + 1)
    n_bad, rows, abc = np.full(3, 77, dtype=np.uint64), np.full(6, 77, dtype=np.uint64), np.full(72, 77, dtype=np.uint64)
    ra = np.stack([f.fr_limbs([3, 5])] * 3)
    proofs, status, n = ct.create_string_buffer(b"M" * (3 * plen), 3 * plen), np.full(3, 77, dtype=np.int32), ct.c_size_t(99)
    sp = status.ctypes.data_as(ct.POINTER(ct.c_int))
    calls = [lambda: L.pm_r1cs_check(gpu_ctx.h, h, vp(xs), vp(ws), 2, 2, api._p(n_bad), api._p(rows), api._p(abc)),
             lambda: L.pm_r1cs_check_batch(gpu_ctx.h, h, 3, vp(xs), vp(ws), 2, 2, api._p(n_bad), api._p(rows), api._p(abc)),
             lambda: L.pm_host_prove(gpu_ctx.h, h, 0, api._p(xs), vp(xs), vp(ws), 2, api._p(ra), proofs, plen, ct.byref(n)),
             lambda: L.pm_host_prove_batch(gpu_ctx.h, h, 0, 3, api._p(xs), vp(xs), vp(ws), 2, api._p(ra), proofs, plen, sp)]
    for call in calls:
        assert call() == PM_ERR_INVALID_ARG
        assert text in gpu_ctx.last_error() and "bitlength" in gpu_ctx.last_error(), gpu_ctx.last_error()
        assert (n_bad == 77).all() and (rows == 77).all() and (abc == 77).all()
        assert proofs.raw == b"M" * (3 * plen) and (status == 77).all() and n.value == 99


# ---- 3. a hand-built system with a decomposition of each kind, a zero divisor and a value without a k-bit form -----------------------------
# columns: 0 one | 1 out (public) | 2 v  3 w  4 g1  5 g2 (given) | 6..9 a0..a3 | 10..12 b0..b2 | 13..15 d0..d2
#   rows 0..9   booleanity of a, b, d
#   row 10: v * 1 = a0 + 2 a1 + 5 + 4 a2 + 8 a3              kind C, a known entry beside the bits
#   row 11: (4c b2 + 7 w + c b0 + 2c b1) * w = g1            kind A, c random, exponents permuted, Bz = w
#   row 12: w * (3 d0 + 6 d1 + 12 d2) = g2                   kind B, c = 3
#   row 13: (a1 + b0) * (d2 + 1) = out                       an ordinary step that reads bits of all three
V, W, G1, G2, A0, B0, D0 = 2, 3, 4, 5, 6, 10, 13


def kinds_system(r, cc):
    from polymath_amd.polymath import R1CS
    boolean = lambda j: ([(1, j)], [(1, 0), (r - 1, j)], [])
    rows = [boolean(j) for j in range(A0, D0 + 3)]
    rows.append(([(1, V)], [(1, 0)], [(1, A0), (2, A0 + 1), (5, 0), (4, A0 + 2), (8, A0 + 3)]))
    rows.append(([(4 * cc % r, B0 + 2), (7, W), (cc, B0), (2 * cc % r, B0 + 1)], [(1, W)], [(1, G1)]))
    rows.append(([(1, W)], [(3, D0), (6, D0 + 1), (12, D0 + 2)], [(1, G2)]))
    rows.append(([(1, A0 + 1), (1, B0)], [(1, D0 + 2), (1, 0)], [(1, 1)]))
    return R1CS(2, 14, [a for a, _, _ in rows], [b for _, b, _ in rows], [c for _, _, c in rows])


def kinds_eval(r, cc, ta, tb, td, w):
    """the assignment in which a, b, d hold ta, tb, td"""
    bits = lambda t, k: [(t >> i) & 1 for i in range(k)]
    out = (((ta >> 1) & 1) + (tb & 1)) * (((td >> 2) & 1) + 1)
    return [1, out], [ta + 5, w, (cc * tb + 7 * w) * w % r, w * 3 * td % r] + bits(ta, 4) + bits(tb, 3) + bits(td, 3)


def kinds_partial(wit):
    return [1, None], list(wit[:4]) + [None] * 10


@pytest.mark.parametrize("curve", BOTH)
def test_kinds_and_stuck(gpu_ctx, curve):
    c = CURVES[curve]
    r = c.r
    from polymath_amd import circuits as PC
    g = PC.SplitMix64(9400)
    cc = g.fr(r)
    s = _cached((curve, "kinds"), lambda: _setup(gpu_ctx, curve, (kinds_system(r, cc),) + tuple(kinds_eval(r, cc, 9, 5, 6, 11)), 9401))
    pm, pk, f = s["pm"], s["pk"], s["f"]
    full = [kinds_eval(r, cc, ta, tb, td, g.fr(r)) for ta, tb, td in ((15, 7, 7), (0, 0, 0), (6, 4, 4))]
    assert [x[1] for x, _ in full] == [4, 0, 2]
    got = pm.solve_batch(pk, [pm.partial_limbs(*kinds_partial(w)) for _, w in full])
    assert got == [(None, x, w) for x, w in full]
    # assignment 0: w = 0, rows 11 and 12 divide by zero; assignment 2: v - 5 = 16 has no 4-bit form, row 10; assignment 1 is complete
    bad_w, bad_v = list(full[0][1]), list(full[2][1])
    bad_w[W - 2] = bad_w[G1 - 2] = bad_w[G2 - 2] = 0
    bad_v[V - 2] = 21
    partials = [kinds_partial(bad_w), kinds_partial(full[1][1]), kinds_partial(bad_v)]
    xs, ws = _stack(s, partials)
    n_bad, rows, stuck, solved = _solve_and_check(s, xs, ws, max_rows=3)
    assert n_bad == [NONE, 0, NONE] and stuck == [11, NONE, 10]
    assert [[int(v) for v in row] for row in rows] == [[11, NONE, NONE], [NONE] * 3, [10, NONE, NONE]]
    assert np.array_equal(solved[1], _full_limbs(s, *full[1]))
    # the columns of a stuck decomposition hold zero; the decompositions beside it are complete
    zero = f.fr_limbs([0] * 3)
    assert np.array_equal(solved[0][B0:B0 + 3], zero) and np.array_equal(solved[0][D0:D0 + 3], zero)
    assert np.array_equal(solved[0][A0:A0 + 4], f.fr_limbs(full[0][1][A0 - 2:A0 + 2]))
    assert np.array_equal(solved[2][A0:A0 + 4], f.fr_limbs([0] * 4)) and np.array_equal(solved[2][B0:], f.fr_limbs(full[2][1][B0 - 2:]))
    assert pm.check_batch(pk, [pm.partial_limbs(*p) for p in partials], max_rows=1, solve=True) == [(NONE, [11]), (0, []), (NONE, [10])]
    # the solving prover: status 1 and zeroed bytes for the two, a proof that verifies for the one between them
    limbs = [pm.partial_limbs(*p) for p in partials]
    r_as = [[31 + i, 41 + i] for i in range(3)]
    proofs, statuses, instances = pm.prove_batch(pk, limbs, r_as, solve=True)
    assert statuses == [PM_ERR_INVALID_ARG, 0, PM_ERR_INVALID_ARG] and instances == [None, full[1][0], None]
    assert proofs[1] == pm.prove_native(pk, f.fr_limbs(full[1][0]), f.fr_limbs(full[1][1]), r_as[1])
    assert pm.verify(pm.make_vk(pk, s["x"], s["z"]), full[1][0][1:], proofs[1])
    rc, data, status = pk.host_prove_batch("merlin", xs, xs, ws, np.stack([f.fr_limbs(ra) for ra in r_as]), solve=True)
    plen = PROOF_LEN[curve]
    assert rc == PM_OK and [int(v) for v in status] == statuses and len(data) == 3 * plen
    assert data[:plen] == bytes(plen) and data[2 * plen:] == bytes(plen) and data[plen:2 * plen] == proofs[1]


# ---- 4. ArxDemo: decompositions in A and in C, XOR rows, recompositions; inputs -> proofs -----------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("width,rounds,rot,check_log,prove_log", [(8, 2, 3, 8, 12), (32, 1, 7, 9, 13)])
def test_arx(gpu_ctx, curve, width, rounds, rot, check_log, prove_log):
    from polymath_amd import circuits as PC
    c = CURVES[curve]
    g = PC.SplitMix64(9500 + width)
    mask = (1 << width) - 1
    inputs = [(mask, mask), (0, 0)] + [(g.next_u64() & mask, g.next_u64() & mask) for _ in range(3)]
    circuits = [PC.ArxDemo(a, b, width, rounds, rot) for a, b in inputs]
    s = _cached((curve, "arx", width), lambda: _setup(gpu_ctx, curve, PC.ArxDemo(1, 2, width, rounds, rot), 9501))
    pm, pk, f, q = s["pm"], s["pk"], s["f"], s["q"]
    assert q.nr == rounds * (5 * width + 6) and q.m0 == 2
    full = [pm._synthesize(ci)[1:] for ci in circuits]                      # the generator's own (instance, witness)
    assert [x[1] for x, _ in full] == [PC.arx_native(a, b, width, rounds, rot) for a, b in inputs]
    xs, ws = _stack(s, [ci.partial(c.r) for ci in circuits])
    count = len(circuits)

    def solved(device):
        if device:
            rc, n_bad, _, _ = pk.r1cs_check_batch(dx.data_ptr(), dw.data_ptr(), 2, on_device=True, count=count, solve=True)
        else:
            rc, n_bad, _, _ = pk.r1cs_check_batch(xs, ws, 2, solve=True)
        assert rc == PM_OK and not n_bad.any(), pm.ctx.last_error()
        stuck, inst = pk.solve_results(count)
        assert [int(v) for v in stuck] == [NONE] * count
        return inst, pk.solved_assignments(count, q.mw).copy()

    one_group = solved(False)
    for i, (x, w) in enumerate(full):
        assert np.array_equal(one_group[1][i], _full_limbs(s, x, w)), i      # word for word the generator's assignment
        assert np.array_equal(one_group[0][i], f.fr_limbs(x))
    # inputs -> proofs: byte-equal to the prover on the completed assignment, and they verify
    r_as = [[51 + i, 61 + i] for i in range(3)]
    limbs = [(xs[i], ws[i]) for i in range(3)]
    proofs, statuses, instances = pm.prove_batch(pk, limbs, r_as, solve=True)
    assert statuses == [0] * 3 and instances == [x for x, _ in full[:3]]
    vk = pm.make_vk(pk, s["x"], s["z"])
    for i in range(3):
        assert pm.verify(vk, full[i][0][1:], proofs[i])
        assert proofs[i] == pm.prove_native(pk, f.fr_limbs(full[i][0]), f.fr_limbs(full[i][1]), r_as[i])
    # several groups and device-resident partial assignments: the same words, the same bytes
    dx, dw = torch.from_numpy(xs.view(np.int64)).cuda(), torch.from_numpy(ws.view(np.int64)).cuda()
    torch.cuda.synchronize()
    ncols = q.m0 + q.mw
    assert 3 * ncols <= 1 << check_log < 4 * ncols                         # the check solves in groups of 3, 2
    gpu_ctx.set_option("msm_max_piece_log", check_log)                     # (restored by conftest)
    for device in (False, True):
        got = solved(device)
        assert np.array_equal(got[0], one_group[0]) and np.array_equal(got[1], one_group[1]), device
    assert 10 * pk.n + 22 <= 1 << prove_log < 2 * (10 * pk.n + 22)         # the prover in groups of 1
    gpu_ctx.set_option("msm_max_piece_log", prove_log)
    assert pm.prove_batch(pk, limbs, r_as, solve=True)[0] == proofs
    got = pm.prove_batch(pk, limbs, r_as, device_ptrs=(dx.data_ptr(), dw.data_ptr()), solve=True)
    assert got[0] == proofs and got[2] == instances
    assert np.array_equal(dx.cpu().numpy().view(np.uint64).reshape(xs.shape), xs)           # the caller's device rows are only read
    assert np.array_equal(dw.cpu().numpy().view(np.uint64).reshape(ws.shape), ws)


# ---- 5. a given value that contradicts its bits: the booleanity row is then a constraint the check reports ------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_boolean_column_fixed_to_two(gpu_ctx, curve):
    """columns 0 one | 1 g (given) | 2 b.  row 0: b (1 - b) = 0; row 1: b * 1 = g, an ordinary row that solves the boolean-pending b"""
    from polymath_amd.polymath import R1CS
    r = CURVES[curve].r
    q = R1CS(1, 2, [[(1, 2)], [(1, 2)]], [[(1, 0), (r - 1, 2)], [(1, 0)]], [[], [(1, 1)]])
    s = _cached((curve, "two"), lambda: _setup(gpu_ctx, curve, (q, [1], [1, 1]), 9600))
    pm, pk = s["pm"], s["pk"]
    partials = [pm.partial_limbs([1], [v, None]) for v in (2, 1, 0, r - 1)]
    assert pm.check_batch(pk, partials, max_rows=4, solve=True) == [(1, [0]), (0, []), (0, []), (1, [0])]
    assert pm.solve_batch(pk, partials)[0] == (None, [1], [2, 2])
