"""GPU: PM_ASSIGNMENT_SOLVE on circuits that test equality -- is-zero pairs (csrc/solve.hip: solve_iszero, k_solve_iszero, the pair
branch of k_solve_chain, the pair lanes of k_solve_inv; host/solve_plan.hpp: opener, closer, KIND_ISZERO).  The bar is equality, word
for word, with Python integers: the generators' own assignments (polymath_amd.circuits: MatchCount, EqChain, native()).

Shapes are the smallest at which each mechanism can differ.  MatchCount with N values is ONE level of N pairs: N = 1 and 31 are walked
by the chain kernel, 32 is the first level with a k_solve_iszero launch of its own, 64 is a whole wave of it, 257 a 256-lane workgroup
and one lane; batches of 1, 3 and 70 are the chain kernel's partial wave and second workgroup and k_solve_iszero's grid y.  Within a
batch assignment i matches everywhere, nowhere or at every other value (i mod 3), so neighbouring lanes take different sides of the
select.  EqChain is len(targets) pairs deep and one wide: one chain launch, at depth 1, 2 and 65, with hits and misses inside one
assignment, and once with a range check on every state so that one launch walks ordinary steps, decompositions and pairs."""
import ctypes as ct

import numpy as np
import pytest
import torch        # noqa: F401  before libpolymath_hip.so is loaded: torch brings its own HIP runtime (tests/ntt_device_child.py)

from oracle.pyref.fields import CURVES
from witness_solve_helpers import BOTH, NONE, PM_ERR_INVALID_ARG, PM_OK, _full_limbs, _setup, _solve, key_cache

pytestmark = pytest.mark.gpu

PM_ERR_REMAINDER_NONZERO = 4
FORMS = ["ark", "circom"]
PROOF_LEN = {"bls12_381": 176, "bn254": 128}
_cached = key_cache()


def _partial_rows(s, circuits, multipliers=False):
    """-> (want, partial): count x (m0 + mw) x 4 words; want = native(), partial = the same with the marker where the device solves"""
    from polymath_amd import api
    r = s["c"].r
    want = np.stack([_full_limbs(s, *ci.native(r)) for ci in circuits])
    inst, wit = circuits[0].partial(r, multipliers=multipliers)
    unknown = np.array([v is None for v in inst + wit])
    partial = want.copy()
    partial[:, unknown] = api.UNKNOWN_LIMBS
    return want, partial


def _match_inputs(g, r, n_values, mode):
    """(values, key) in which every value, no value or every other value equals the key"""
    key = g.fr(r)
    hit = {0: lambda j: True, 1: lambda j: False, 2: lambda j: j % 2 == 0}[mode]
    return [key if hit(j) else (key + 1 + g.next_u64()) % r for j in range(n_values)], key


# ---- 1. MatchCount: one level of N pairs, at the chain / level threshold and the wave and workgroup edges of k_solve_iszero ----------------
@pytest.mark.parametrize("curve,form,n_values", [("bls12_381", "ark", n) for n in (1, 31, 32, 64, 257)] +
                         [(curve, form, n) for curve in BOTH for form in FORMS for n in (31, 32) if (curve, form) != ("bls12_381", "ark")] +
                         [("bn254", "circom", 1), ("bn254", "circom", 257)])
def test_match_count(gpu_ctx, curve, form, n_values):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    s = _cached((curve, "match", form, n_values), lambda: _setup(gpu_ctx, curve, PC.MatchCount(list(range(n_values)), 3, form), 9700 + n_values))
    q = s["q"]
    assert (q.m0, q.mw, q.nr) == (2, 1 + 3 * n_values, (3 if form == "ark" else 2) * n_values + 1)
    g = PC.SplitMix64(9800 + n_values)
    for count in (1, 3, 70):
        inputs = [_match_inputs(g, r, n_values, 2 if count == 1 else i % 3) for i in range(count)]
        circuits = [PC.MatchCount(values, key, form) for values, key in inputs]
        want, partial = _partial_rows(s, circuits)
        counts = [s["f"].fr_int(row[1]) for row in want]
        assert counts == [{0: n_values, 1: 0, 2: (n_values + 1) // 2}[2 if count == 1 else i % 3] for i in range(count)]
        n_bad, _, stuck, full = _solve(s, partial)
        assert n_bad == [0] * count and stuck == [NONE] * count, (count, n_bad, stuck)
        assert np.array_equal(full, want), count


# ---- 2. EqChain: a chain of pairs, each of which reads the flag before it; with bits, a decomposition between them ---------------------------
@pytest.mark.parametrize("curve,form", [("bls12_381", "ark"), ("bn254", "circom")])
@pytest.mark.parametrize("depth,bits", [(1, 0), (2, 0), (65, 0), (2, 8), (9, 24)])
def test_eq_chain(gpu_ctx, curve, form, depth, bits):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    s = _cached((curve, "chain", form, depth, bits), lambda: _setup(gpu_ctx, curve, PC.EqChain(3, PC.eq_chain_targets(3, [True] * depth, r), form, bits=bits), 9900 + depth))
    q = s["q"]
    assert q.nr == ((4 if form == "ark" else 3) + (bits + 1 if bits else 0)) * depth and q.m0 == 2
    g = PC.SplitMix64(9950 + depth + bits)
    for count in (1, 3, 70):
        circuits, seen = [], set()
        for i in range(count):
            x = 1 + g.next_u64() % 50 if bits else g.fr(r)
            hits = [(i + j) % 3 != 1 for j in range(depth)] if depth > 1 else [i % 2 == 0]      # hit and miss within one assignment
            seen.update(hits)
            circuits.append(PC.EqChain(x, PC.eq_chain_targets(x, hits, r), form, bits=bits))
        assert seen == ({True, False} if count > 1 or depth > 1 else {True})
        want, partial = _partial_rows(s, circuits)
        n_bad, _, stuck, full = _solve(s, partial)
        assert n_bad == [0] * count and stuck == [NONE] * count, (count, n_bad, stuck)
        assert np.array_equal(full, want), count


# ---- 3. inputs -> proofs, under several groupings, from device pointers, and pm_host_prove at count 1 ----------------------------------------
@pytest.mark.parametrize("curve,form", [("bls12_381", "ark"), ("bls12_381", "circom"), ("bn254", "ark")])
def test_end_to_end(gpu_ctx, curve, form):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    n_values, count = 40, 5
    s = _cached((curve, "match", form, n_values), lambda: _setup(gpu_ctx, curve, PC.MatchCount(list(range(n_values)), 3, form), 9700 + n_values))
    pm, pk, f, q = s["pm"], s["pk"], s["f"], s["q"]
    g = PC.SplitMix64(10000)
    circuits = [PC.MatchCount(*_match_inputs(g, r, n_values, i % 3), form) for i in range(count)]
    full = [ci.native(r) for ci in circuits]
    want, partial = _partial_rows(s, circuits)
    xs, ws = np.ascontiguousarray(partial[:, :q.m0]), np.ascontiguousarray(partial[:, q.m0:])
    r_as = [[71 + i, 81 + i] for i in range(count)]
    limbs = [(xs[i], ws[i]) for i in range(count)]
    proofs, statuses, instances = pm.prove_batch(pk, limbs, r_as, solve=True)
    assert statuses == [0] * count and instances == [x for x, _ in full]
    vk = pm.make_vk(pk, s["x"], s["z"])
    for i in range(count):
        assert pm.verify(vk, full[i][0][1:], proofs[i])
        assert proofs[i] == pm.prove_native(pk, f.fr_limbs(full[i][0]), f.fr_limbs(full[i][1]), r_as[i])
    rc, one = pk.host_prove("merlin", xs[1], xs[1], ws[1], f.fr_limbs(r_as[1]), solve=True)
    assert rc == PM_OK and one == proofs[1]
    # several groups and device-resident partial assignments: the same words, the same bytes
    dx, dw = torch.from_numpy(xs.view(np.int64)).cuda(), torch.from_numpy(ws.view(np.int64)).cuda()
    torch.cuda.synchronize()
    ncols = q.m0 + q.mw
    check_log = (2 * ncols - 1).bit_length()
    assert 2 * ncols <= 1 << check_log < 4 * ncols                         # the check solves in groups of 2 or 3
    gpu_ctx.set_option("msm_max_piece_log", check_log)                     # (restored by conftest)
    for device in (False, True):
        if device:
            rc, n_bad, _, _ = pk.r1cs_check_batch(dx.data_ptr(), dw.data_ptr(), 2, on_device=True, count=count, solve=True)
        else:
            rc, n_bad, _, _ = pk.r1cs_check_batch(xs, ws, 2, solve=True)
        assert rc == PM_OK and not n_bad.any(), pm.ctx.last_error()
        assert np.array_equal(pk.solved_assignments(count, q.mw), want), device
    prove_log = (10 * pk.n + 22 - 1).bit_length()
    assert 10 * pk.n + 22 <= 1 << prove_log < 2 * (10 * pk.n + 22)         # the prover in groups of 1
    gpu_ctx.set_option("msm_max_piece_log", prove_log)
    assert pm.prove_batch(pk, limbs, r_as, solve=True)[0] == proofs
    got = pm.prove_batch(pk, limbs, r_as, device_ptrs=(dx.data_ptr(), dw.data_ptr()), solve=True)
    assert got[0] == proofs and got[2] == instances
    assert np.array_equal(dx.cpu().numpy().view(np.uint64).reshape(xs.shape), xs)           # the caller's device rows are only read
    assert np.array_equal(dw.cpu().numpy().view(np.uint64).reshape(ws.shape), ws)


# ---- 4. the escape hatch: the caller gives the multipliers (arkworks writes 1 where the values are equal), only the flags are solved ---------
@pytest.mark.parametrize("curve,form", [("bls12_381", "ark"), ("bn254", "circom")])
def test_multiplier_given(gpu_ctx, curve, form):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    n_values, count = 40, 3
    s = _cached((curve, "match", form, n_values), lambda: _setup(gpu_ctx, curve, PC.MatchCount(list(range(n_values)), 3, form), 9700 + n_values))
    pm, pk, f, q = s["pm"], s["pk"], s["f"], s["q"]
    g = PC.SplitMix64(10100)
    inputs = [_match_inputs(g, r, n_values, i % 3) for i in range(count)]
    ark = [PC.MatchCount(values, key, form, free=1) for values, key in inputs]
    want, partial = _partial_rows(s, ark, multipliers=True)
    zero_want, _ = _partial_rows(s, [PC.MatchCount(values, key, form) for values, key in inputs])
    assert not np.array_equal(want[0], zero_want[0]) and np.array_equal(want[1], zero_want[1])      # the conventions differ where values match
    n_bad, _, stuck, full = _solve(s, partial)
    assert n_bad == [0] * count and stuck == [NONE] * count and np.array_equal(full, want)
    xs, ws = np.ascontiguousarray(partial[:, :q.m0]), np.ascontiguousarray(partial[:, q.m0:])
    r_as = [[91 + i, 101 + i] for i in range(count)]
    proofs, statuses, _ = pm.prove_batch(pk, [(xs[i], ws[i]) for i in range(count)], r_as, solve=True)
    assert statuses == [0] * count
    for i, ci in enumerate(ark):                                             # byte-equal to the host-synthesised arkworks-convention assignment's
        inst, wit = ci.native(r)
        assert proofs[i] == pm.prove_native(pk, f.fr_limbs(inst), f.fr_limbs(wit), r_as[i])


# ---- 5. d = 0 with a closer whose constant side is not zero: an ordinary failing row, not a solver error -------------------------------------
# columns: 0 one | 1 out (public) | 2 a  3 b  4 k (given) | 5 flag  6 m
#   row 0: (a - b) * m = flag        row 1: (a - b) * (1 - flag) = k        row 2: flag * 1 = out
def failing_system(r):
    from polymath_amd.polymath import R1CS
    lc = [(1, 2), (r - 1, 3)]
    return R1CS(2, 5, [lc, lc, [(1, 5)]], [[(1, 6)], [(1, 0), (r - 1, 5)], [(1, 0)]], [[(1, 5)], [(1, 4)], [(1, 1)]])


@pytest.mark.parametrize("curve", BOTH)
def test_failing_closer(gpu_ctx, curve):
    r = CURVES[curve].r
    s = _cached((curve, "failing"), lambda: _setup(gpu_ctx, curve, (failing_system(r), [1, 1], [9, 4, 0, 1, pow(5, r - 2, r)]), 10200))
    pm, pk, f = s["pm"], s["pk"], s["f"]
    # a != b, k = 0: neq = 1;  a == b, k = 7: flag = 0 by the opener, and the closer reads 0 = 7;  a != b, k = 10: 5 (1 - flag) = 10, flag = -1
    partials = [pm.partial_limbs([1, None], [9, 4, 0, None, None]), pm.partial_limbs([1, None], [6, 6, 7, None, None]), pm.partial_limbs([1, None], [9, 4, 10, None, None])]
    inv5 = pow(5, r - 2, r)
    assert pm.solve_batch(pk, partials) == [(None, [1, 1], [9, 4, 0, 1, inv5]), (None, [1, 0], [6, 6, 7, 0, 0]), (None, [1, r - 1], [9, 4, 10, r - 1, (r - 1) * inv5 % r])]
    assert pm.check_batch(pk, partials, max_rows=2, solve=True) == [(0, []), (1, [1]), (0, [])]
    r_as = [[11 + i, 21 + i] for i in range(3)]
    proofs, statuses, instances = pm.prove_batch(pk, partials, r_as, solve=True)
    assert statuses == [0, PM_ERR_REMAINDER_NONZERO, 0] and proofs[1] is None and instances == [[1, 1], [1, 0], [1, r - 1]]
    assert proofs[0] == pm.prove_native(pk, f.fr_limbs([1, 1]), f.fr_limbs([9, 4, 0, 1, inv5]), r_as[0])      # the neighbours are untouched
    assert pm.verify(pm.make_vk(pk, s["x"], s["z"]), [r - 1], proofs[2])
    x, w = partials[1]
    rc, _ = pk.host_prove("merlin", x, x, w, f.fr_limbs(r_as[1]), solve=True)
    assert rc == PM_ERR_REMAINDER_NONZERO


# ---- 6. refused through the C ABI: an opener nothing closes, a closer with another known side -------------------------------------------------
# columns: 0 one | 1 out | 2 a  3 b (given) | 4 flag  5 m.   Row 0: the opener.  Row 1: out * 1 = a, which names neither.
#   unclosed: row 2 is a check row.       other side: row 2 is (a - 2 b) * (1 - flag) = 0
def refused_system(r, which):
    from polymath_amd.polymath import R1CS
    lc = [(1, 2), (r - 1, 3)]
    last = ([(1, 2)], [(1, 0)], [(1, 2)]) if which == "unclosed" else ([(1, 2), (r - 2, 3)], [(1, 0), (r - 1, 4)], [])
    return R1CS(2, 4, [lc, [(1, 1)], last[0]], [[(1, 5)], [(1, 0)], last[1]], [[(1, 4)], [(1, 2)], last[2]])


@pytest.mark.parametrize("which,needle", [("unclosed", "no later row closes it"), ("other side", "row 2: its known side")])
def test_refused_structures(gpu_ctx, which, needle):
    from polymath_amd import api
    curve = "bls12_381"
    r = CURVES[curve].r
    satisfying = [8, 8, 0, 0] if which == "unclosed" else [8, 4, 1, pow(4, r - 2, r)]
    s = _cached((curve, "refused", which), lambda: _setup(gpu_ctx, curve, (refused_system(r, which), [1, 8], satisfying), 10300))
    pm, pk, f = s["pm"], s["pk"], s["f"]
    L, vp, plen = gpu_ctx.L, (lambda a: a.ctypes.data_as(ct.c_void_p)), PROOF_LEN[curve]
    pairs = [pm.partial_limbs([1, None], [8 + i, 5, None, None]) for i in range(3)]
    xs, ws = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    text = "row 0: two or more unknowns (columns 5 and 4)"
    n_bad, rows, abc = np.full(3, 77, dtype=np.uint64), np.full(6, 77, dtype=np.uint64), np.full(72, 77, dtype=np.uint64)
    ra = np.stack([f.fr_limbs([3, 5])] * 3)
    proofs, status, n = ct.create_string_buffer(b"M" * (3 * plen), 3 * plen), np.full(3, 77, dtype=np.int32), ct.c_size_t(99)
    sp = status.ctypes.data_as(ct.POINTER(ct.c_int))
    calls = [lambda: L.pm_r1cs_check(gpu_ctx.h, pk.h, vp(xs), vp(ws), 2, 2, api._p(n_bad), api._p(rows), api._p(abc)),
             lambda: L.pm_r1cs_check_batch(gpu_ctx.h, pk.h, 3, vp(xs), vp(ws), 2, 2, api._p(n_bad), api._p(rows), api._p(abc)),
             lambda: L.pm_host_prove(gpu_ctx.h, pk.h, 0, api._p(xs), vp(xs), vp(ws), 2, api._p(ra), proofs, plen, ct.byref(n)),
             lambda: L.pm_host_prove_batch(gpu_ctx.h, pk.h, 0, 3, api._p(xs), vp(xs), vp(ws), 2, api._p(ra), proofs, plen, sp)]
    for call in calls:
        assert call() == PM_ERR_INVALID_ARG
        assert text in gpu_ctx.last_error() and needle in gpu_ctx.last_error(), gpu_ctx.last_error()
        assert (n_bad == 77).all() and (rows == 77).all() and (abc == 77).all()
        assert proofs.raw == b"M" * (3 * plen) and (status == 77).all() and n.value == 99
    # the context is as usable as before and the refused pattern did not stay in the plan cache: with m given the flag is an ordinary
    # step of row 0, and the refused pattern is refused again after it
    given = pm.partial_limbs([1, None], [8, 5, None, pow(3, r - 2, r)])
    assert pm.solve_batch(pk, [given]) == [(None, [1, 8], [8, 5, 1, pow(3, r - 2, r)])]
    assert calls[1]() == PM_ERR_INVALID_ARG and text in gpu_ctx.last_error()
