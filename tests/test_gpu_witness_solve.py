"""GPU: PM_ASSIGNMENT_SOLVE -- partial assignments completed on the device by forward propagation through the key's constraint rows
(csrc/solve.hip, host/solve_plan.hpp), then checked or proved.  The bar is equality, word for word, with Python integers: the
circuits' own assignments from oracle.pyref.circuits (mimc_circuit / mimc_native, synthetic_r1cs, first_entry_dot) and pow(a, -1, r).

Shapes are the smallest at which each mechanism can differ.  The chain kernel runs one lane per assignment in 64-lane workgroups:
1, 3 and 70 assignments of MiMC-322 (644 levels of width 1) are a partial wave and two workgroups.  The level kernel runs 256-lane
workgroups over the steps of one level: the diagonal at nr = 1, 64, 257, 500 is a partial wave, a whole wave, a workgroup edge and
two workgroups with a partial last one.  synthetic_r1cs at nr = 2000 mixes chains of narrow levels with sub-workgroup level launches
(widths 3, 7, 9, 16, 19, 17, 26, 29, 34, ... 162 ... 17 around the threshold of 32); nr = 20000 adds multi-workgroup levels."""
import ctypes as ct

import numpy as np
import pytest
import torch        # noqa: F401  before libpolymath_hip.so is loaded: torch brings its own HIP runtime (tests/ntt_device_child.py)

from oracle.pyref import circuits as CI
from oracle.pyref.fields import CURVES
from witness_solve_helpers import BOTH, NONE, PM_ERR_INVALID_ARG, PM_OK, key_cache

pytestmark = pytest.mark.gpu

PM_ERR_REMAINDER_NONZERO, PM_ERR_STATE = 4, 8
_cached = key_cache()


def _setup(gpu_ctx, curve, q, inst, wit, seed):
    from polymath_amd import polymath as PM
    c = CURVES[curve]
    g = CI.SplitMix64(seed)
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    x, z = g.fr(c.r), g.fr(c.r)
    pk = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), inst, wit), x, z)
    return dict(pm=pm, pk=pk, q=q, inst=inst, wit=wit, x=x, z=z, f=pm.field, c=c)


def _stack(s, partials):
    pairs = [s["pm"].partial_limbs(i, w) for i, w in partials]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _full_limbs(s, inst, wit):
    return np.concatenate([s["f"].fr_limbs(inst), s["f"].fr_limbs(wit)])


def _solve_and_check(s, partials, max_rows=2, **kw):
    """r1cs_check_batch(solve=True) on host limbs -> (n_bad, rows, stuck words, instances, completed x || w rows)"""
    xs, ws = _stack(s, partials)
    rc, n_bad, rows, _ = s["pk"].r1cs_check_batch(xs, ws, max_rows, solve=True, **kw)
    assert rc == PM_OK, s["pm"].ctx.last_error()
    stuck, inst = s["pk"].solve_results(len(partials))
    return n_bad, rows, stuck, inst, s["pk"].solved_assignments(len(partials), s["q"].mw)


# ---- circuits -----------------------------------------------------------------------------------------------------------------------
MIMC_ROUNDS = 322


def _mimc_consts(c):
    g = CI.SplitMix64(7300)
    return [g.fr(c.r) for _ in range(MIMC_ROUNDS)]


def _mimc_key(gpu_ctx, curve):
    def make():
        c = CURVES[curve]
        q, inst, wit = CI.mimc_circuit(c, 5, 7, _mimc_consts(c))
        assert len(q.a) == 644 and q.m0 + q.mw == 647
        return _setup(gpu_ctx, curve, q, inst, wit, 7400)
    return _cached((curve, "mimc"), make)


def _mimc_rows(c, count, seed):
    g = CI.SplitMix64(seed)
    consts = _mimc_consts(c)
    out = []
    for _ in range(count):
        xl, xr = g.fr(c.r), g.fr(c.r)
        _, inst, wit = CI.mimc_circuit(c, xl, xr, consts)
        assert inst[1] == CI.mimc_native(c, xl, xr, consts)
        out.append((inst, wit, ([1, None], [xl, xr] + [None] * (len(wit) - 2))))
    return out


def diagonal(c, nr):
    """row r is  w[r] * 1 = w[nr + r]"""
    q = CI.R1CS(1, 2 * nr, [[(1, 1 + r)] for r in range(nr)], [[(1, 0)] for _ in range(nr)], [[(1, 1 + nr + r)] for r in range(nr)])
    return q


def _diag_key(gpu_ctx, curve, nr):
    def make():
        q = diagonal(CURVES[curve], nr)
        return _setup(gpu_ctx, curve, q, [1], [3 + r for r in range(nr)] * 2, 7500 + nr)
    return _cached((curve, "diag", nr), make)


def _synth_key(gpu_ctx, curve, nr):
    def make():
        q, inst, wit = CI.synthetic_r1cs(CURVES[curve], nr)
        return _setup(gpu_ctx, curve, q, inst, wit, 7600 + nr)
    return _cached((curve, "synth", nr), make)


def synth_eval(c, q, w0, w1):
    """the gates of synthetic_r1cs evaluated in row order from other seed witnesses"""
    z = [None] * (q.m0 + q.mw)
    z[0], z[2], z[3] = 1, w0, w1
    for ra, rb, rc in zip(q.a, q.b, q.c):
        (alpha, p), (beta, qq), (one, t) = ra[0], rb[0], rc[0]
        assert one == 1
        z[t] = (alpha * z[p] % c.r) * (beta * z[qq] % c.r) % c.r
    return z[:2], z[2:]


# columns: 0 one | 1 out (public) | 2 a  3 c  4 inv  5 q  6 s  7 e  8 pad (no row names it)
#   row 0: (3 inv) a = 1      inv in A          row 1: a (5 q) = c      q in B          row 2: inv q = s      s in C
#   row 3: (s + 1) 1 = out    out in C          row 4: a a = e          a check row when a and e are given
A_, C_, INV, Q_, S_, E_, PAD = 2, 3, 4, 5, 6, 7, 8


def kinds_system():
    return CI.R1CS(2, 7, [[(3, INV)], [(1, A_)], [(1, INV)], [(1, S_), (1, 0)], [(1, A_)]],
                   [[(1, A_)], [(5, Q_)], [(1, Q_)], [(1, 0)], [(1, A_)]],
                   [[(1, 0)], [(1, C_)], [(1, S_)], [(1, 1)], [(1, E_)]])


def kinds_eval(c, a, cc, e=None, pad=9):
    r = c.r
    inv = pow(a, -1, r) * pow(3, -1, r) % r
    q = cc * pow(a, -1, r) * pow(5, -1, r) % r
    s = inv * q % r
    return [1, (s + 1) % r], [a, cc, inv, q, s, a * a % r if e is None else e, pad]


def kinds_partial(a, cc, e, pad=9):
    return [1, None], [a, cc, None, None, None, e, pad]


def _kinds_key(gpu_ctx, curve):
    def make():
        inst, wit = kinds_eval(CURVES[curve], 11, 13)
        return _setup(gpu_ctx, curve, kinds_system(), inst, wit, 7700)
    return _cached((curve, "kinds"), make)


# ---- 1. the chain kernel: MiMC-322, depth 644, width 1 --------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_chain_mimc(gpu_ctx, curve):
    s = _mimc_key(gpu_ctx, curve)
    pm, pk, c = s["pm"], s["pk"], s["c"]
    rows = _mimc_rows(c, 70, 8100)
    for count in (1, 3, 70):
        got = pm.solve_batch(pk, [pm.partial_limbs(*p) for _, _, p in rows[:count]])
        assert got == [(None, inst, wit) for inst, wit, _ in rows[:count]]
        stuck, inst = pk.solve_results(count)
        assert [int(v) for v in stuck] == [NONE] * count
        assert [[pm.field.fr_int(v) for v in inst[i]] for i in range(count)] == [r[0] for r in rows[:count]]      # [1, mimc_native]
    t = pm.ctx.timings()
    assert t["ntt"] > 0 and all(v == 0 for k, v in t.items() if k not in ("witness_map", "ntt"))     # slot 1: the solve kernels
    # check_batch on the completed assignments: all satisfied; and with max_rows > 0
    assert pm.check_batch(pk, [pm.partial_limbs(*p) for _, _, p in rows[:3]], max_rows=4, solve=True) == [(0, [])] * 3


# ---- 2. the level kernel: one wide level ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("nr", [1, 64, 257, 500])
def test_level_diagonal(gpu_ctx, curve, nr):
    s = _diag_key(gpu_ctx, curve, nr)
    c = s["c"]
    g = CI.SplitMix64(8200 + nr)
    halves = [[g.fr(c.r) for _ in range(nr)] for _ in range(3)]
    n_bad, _, stuck, inst, full = _solve_and_check(s, [([1], h + [None] * nr) for h in halves])
    assert [int(v) for v in n_bad] == [0, 0, 0] and [int(v) for v in stuck] == [NONE] * 3
    for i, h in enumerate(halves):
        assert np.array_equal(full[i], _full_limbs(s, [1], h + h)), i
        assert np.array_equal(inst[i], s["f"].fr_limbs([1]))


# ---- 3. both kernels, kind sorting, partial last blocks -------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("nr", [2000, 20000])
def test_synthetic(gpu_ctx, curve, nr):
    s = _synth_key(gpu_ctx, curve, nr)
    c, q = s["c"], s["q"]
    own = (s["inst"], s["wit"])
    assert synth_eval(c, q, s["wit"][0], s["wit"][1]) == (list(own[0]), list(own[1]))
    other = synth_eval(c, q, 12345, c.r - 2)
    partials = [([1, None], [w[0], w[1]] + [None] * (q.mw - 2)) for _, w in (own, other)]
    n_bad, _, stuck, inst, full = _solve_and_check(s, partials)
    assert [int(v) for v in n_bad] == [0, 0] and [int(v) for v in stuck] == [NONE, NONE]
    for i, (x, w) in enumerate((own, other)):
        assert np.array_equal(full[i], _full_limbs(s, x, w)), i          # the completed x || w is the generator's
        assert np.array_equal(inst[i], s["f"].fr_limbs(x))


# ---- 4. kinds A and B, a coefficient to invert, stuck rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_kinds_and_stuck(gpu_ctx, curve):
    s = _kinds_key(gpu_ctx, curve)
    pm, pk, c, f = s["pm"], s["pk"], s["c"], s["f"]
    g = CI.SplitMix64(8400)
    vals = [(g.fr(c.r), g.fr(c.r)) for _ in range(3)]
    got = pm.solve_batch(pk, [pm.partial_limbs(*kinds_partial(a, cc, a * a % c.r)) for a, cc in vals])
    assert got == [(None,) + tuple(kinds_eval(c, a, cc)) for a, cc in vals]
    assert got[0][2][INV - 2] == pow(3 * vals[0][0], -1, c.r)
    # a = 0 in assignment 1: rows 0 and 1 divide by zero, the smaller is reported; the neighbours are complete
    partials = [kinds_partial(a, cc, a * a % c.r) for a, cc in vals]
    partials[1] = kinds_partial(0, vals[1][1], 0)
    n_bad, rows, stuck, inst, full = _solve_and_check(s, partials, max_rows=3, residuals=True)
    assert [int(v) for v in n_bad] == [0, NONE, 0]
    assert [int(v) for v in rows[1]] == [0, NONE, NONE] and [int(v) for v in stuck] == [NONE, 0, NONE]
    assert not inst[1].any()
    for i in (0, 2):
        assert np.array_equal(full[i], _full_limbs(s, *kinds_eval(c, *vals[i]))) and [int(v) for v in rows[i]] == [NONE] * 3
    assert pm.solve_batch(pk, [pm.partial_limbs(*p) for p in partials])[1] == (0, None, None)
    rc, n1, rows1, abc1 = pk.r1cs_check(*pm.partial_limbs(*partials[1]), 3, residuals=True, solve=True)
    assert (rc, n1, [int(v) for v in rows1]) == (PM_OK, NONE, [0, NONE, NONE]) and not abc1.any()
    rc, n1, rows1, _ = pk.r1cs_check(*pm.partial_limbs(*kinds_partial(0, 0, 0)), 0, solve=True)       # 0 / 0 is stuck too; count only
    assert (rc, n1) == (PM_OK, NONE) and int(pk.solve_results(1)[0][0]) == 0


@pytest.mark.parametrize("curve", BOTH)
def test_prove_statuses_follow_the_check(gpu_ctx, curve):
    """four partial assignments: complete, stuck, complete, complete with a given e != a^2 (row 4 fails): the solving check reports
    n_bad > 0 exactly where the solving prover returns status 4, and the stuck one gets status 1 and zeroed bytes"""
    s = _kinds_key(gpu_ctx, curve)
    pm, pk, c, f = s["pm"], s["pk"], s["c"], s["f"]
    vals = [(21, 22), (0, 5), (23, 24), (25, 26)]
    partials = [kinds_partial(a, cc, a * a % c.r) for a, cc in vals]
    partials[3] = kinds_partial(25, 26, 1)
    limbs = [pm.partial_limbs(*p) for p in partials]
    checks = pm.check_batch(pk, limbs, max_rows=1, solve=True)
    assert checks[0] == (0, []) and checks[2] == (0, []) and checks[3] == (1, [4]) and checks[1][0] == NONE
    r_as = [[31 + i, 41 + i] for i in range(4)]
    proofs, statuses, instances = pm.prove_batch(pk, limbs, r_as, solve=True)
    assert statuses == [0, PM_ERR_INVALID_ARG, 0, PM_ERR_REMAINDER_NONZERO]
    assert proofs[1] is None and proofs[3] is None and instances[1] is None
    vk = pm.make_vk(pk, s["x"], s["z"])
    for i in (0, 2):
        inst, wit = kinds_eval(c, *vals[i])
        assert instances[i] == inst and pm.verify(vk, inst[1:], proofs[i])
        assert proofs[i] == pm.prove_native(pk, f.fr_limbs(inst), f.fr_limbs(wit), r_as[i])
    assert instances[3] == kinds_eval(c, 25, 26)[0]
    with pytest.raises(Exception):
        pk.solved_assignments(4, 7)                                      # tap 10 after a prove call: PM_ERR_STATE
    # pm_host_prove: the batch with count 1
    x, w = limbs[0]
    rc, one = pk.host_prove("merlin", x, x, w, f.fr_limbs(r_as[0]), solve=True)
    assert rc == PM_OK and one == proofs[0]
    x, w = limbs[1]
    rc, one = pk.host_prove("merlin", x, x, w, f.fr_limbs(r_as[1]), solve=True)
    assert rc == PM_ERR_INVALID_ARG and "row 0" in pm.ctx.last_error() and int(pk.solve_results(1)[0][0]) == 0
    x, w = limbs[3]
    rc, one = pk.host_prove("merlin", x, x, w, f.fr_limbs(r_as[3]), solve=True)
    assert rc == PM_ERR_REMAINDER_NONZERO
    proofs1, statuses1, _ = pm.prove_batch(pk, limbs[1:2], r_as[1:2], solve=True)       # count == 1: stuck is the row's status
    assert statuses1 == [PM_ERR_INVALID_ARG] and proofs1 == [None]


# ---- 5. what the solver refuses: PM_ERR_INVALID_ARG, outputs untouched, pm_last_error names the row or column -------------------------------
def test_structure_errors(gpu_ctx):
    from polymath_amd import api
    s = _kinds_key(gpu_ctx, "bls12_381")
    pm, pk, c, f = s["pm"], s["pk"], s["c"], s["f"]
    L, vp = gpu_ctx.L, lambda a: a.ctypes.data_as(ct.c_void_p)
    good = kinds_partial(21, 22, 441)
    two = ([1, None], [None, 22, None, None, None, 441, 9])                  # a and inv unknown: row 0 has two unknowns
    col0 = ([None, None], good[1])
    undetermined = ([1, None], good[1][:6] + [None])                        # pad: no row names it
    differs = ([1, None], [21, 22, None, None, None, None, 9])              # marks e as well
    cases = [("row 0", [two] * 3), ("column 0", [col0] * 3), ("column 8", [undetermined] * 3), ("assignment 2 differs from assignment 0 at column 7", [good, good, differs])]
    for text, partials in cases:
        xs, ws = _stack(s, partials)
        n_bad, rows, abc = np.full(3, 77, dtype=np.uint64), np.full(6, 77, dtype=np.uint64), np.full(72, 77, dtype=np.uint64)
        assert L.pm_r1cs_check_batch(gpu_ctx.h, pk.h, 3, vp(xs), vp(ws), 2, 2, api._p(n_bad), api._p(rows), api._p(abc)) == PM_ERR_INVALID_ARG, text
        assert text in gpu_ctx.last_error(), (text, gpu_ctx.last_error())
        assert (n_bad == 77).all() and (rows == 77).all() and (abc == 77).all(), text
        ra = np.stack([f.fr_limbs([3, 5])] * 3)
        proofs, status = ct.create_string_buffer(b"M" * (3 * 176), 3 * 176), np.full(3, 77, dtype=np.int32)
        sp = status.ctypes.data_as(ct.POINTER(ct.c_int))
        assert L.pm_host_prove_batch(gpu_ctx.h, pk.h, 0, 3, api._p(xs), vp(xs), vp(ws), 2, api._p(ra), proofs, 176, sp) == PM_ERR_INVALID_ARG
        assert text in gpu_ctx.last_error() and proofs.raw == b"M" * (3 * 176) and (status == 77).all(), text
        if "assignment" not in text:                                         # one assignment: pm_r1cs_check, pm_host_prove, a batch of one
            assert L.pm_r1cs_check(gpu_ctx.h, pk.h, vp(xs), vp(ws), 2, 2, api._p(n_bad), api._p(rows), api._p(abc)) == PM_ERR_INVALID_ARG
            n = ct.c_size_t(99)
            assert L.pm_host_prove(gpu_ctx.h, pk.h, 0, api._p(xs), vp(xs), vp(ws), 2, api._p(ra), proofs, 176, ct.byref(n)) == PM_ERR_INVALID_ARG
            assert L.pm_host_prove_batch(gpu_ctx.h, pk.h, 0, 1, api._p(xs), vp(xs), vp(ws), 2, api._p(ra), proofs, 176, sp) == PM_ERR_INVALID_ARG
            assert text in gpu_ctx.last_error() and (n_bad == 77).all() and proofs.raw == b"M" * (3 * 176) and (status == 77).all() and n.value == 99, text
    # a flag bit outside the two, a sharded key
    xs, ws = _stack(s, [good] * 3)
    n_bad = np.full(3, 77, dtype=np.uint64)
    for flags in (4, 6, 8, 1 << 8):
        assert L.pm_r1cs_check_batch(gpu_ctx.h, pk.h, 3, vp(xs), vp(ws), flags, 0, api._p(n_bad), None, None) == PM_ERR_INVALID_ARG
    from polymath_amd import polymath as PM
    q = s["q"]
    half = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), s["inst"], s["wit"]), 123, 456, 0, 2)
    assert L.pm_r1cs_check_batch(gpu_ctx.h, half.h, 3, vp(xs), vp(ws), 2, 0, api._p(n_bad), None, None) == PM_ERR_INVALID_ARG
    n = ct.c_size_t(0)
    assert L.pm_host_prove(gpu_ctx.h, half.h, 0, api._p(xs), vp(xs), vp(ws), 2, api._p(f.fr_limbs([3, 5])), ct.create_string_buffer(176), 176, ct.byref(n)) == PM_ERR_INVALID_ARG
    half.free()
    assert (n_bad == 77).all()
    # the context is as usable as before, and the refused patterns did not stay in the plan cache
    assert pm.solve_batch(pk, [pm.partial_limbs(*good)]) == [(None,) + tuple(kinds_eval(c, 21, 22))]


def test_taps_need_a_solving_call():
    from polymath_amd import api
    ctx = api.Context(0)
    out, n = np.zeros(8, dtype=np.uint64), ct.c_size_t(0)
    for which in (9, 10):
        assert ctx.L.pm_prove_tap(ctx.h, which, api._p(out), 2, ct.byref(n)) == PM_ERR_STATE
    ctx.close()


# ---- 6. groups: the same words however the batch is split, from host and from device pointers ----------------------------------------------
def test_groups(gpu_ctx):
    s = _synth_key(gpu_ctx, "bls12_381", 2000)
    pm, pk, c, q = s["pm"], s["pk"], s["c"], s["q"]
    count = 5
    seeds = [(s["wit"][0], s["wit"][1])] + [(100 + i, c.r - 1 - i) for i in range(1, count)]
    xs, ws = _stack(s, [([1, None], [a, b] + [None] * (q.mw - 2)) for a, b in seeds])
    dx, dw = torch.from_numpy(xs.view(np.int64)).cuda(), torch.from_numpy(ws.view(np.int64)).cuda()
    torch.cuda.synchronize()

    def run(device):
        if device:
            rc, n_bad, rows, _ = pk.r1cs_check_batch(dx.data_ptr(), dw.data_ptr(), 2, on_device=True, count=count, solve=True)
        else:
            rc, n_bad, rows, _ = pk.r1cs_check_batch(xs, ws, 2, solve=True)
        assert rc == PM_OK and not n_bad.any()
        stuck, inst = pk.solve_results(count)
        return stuck, inst, pk.solved_assignments(count, q.mw).copy()

    one_group = run(False)
    assert np.array_equal(one_group[2][0], _full_limbs(s, s["inst"], s["wit"]))
    assert np.array_equal(one_group[2][3], _full_limbs(s, *synth_eval(c, q, *seeds[3])))
    assert q.m0 + q.mw == 2003 and 2 * 2003 <= 1 << 12 < 3 * 2003
    gpu_ctx.set_option("msm_max_piece_log", 12)                # groups of 2, 2, 1 (restored by conftest)
    for device in (False, True):
        got = run(device)
        assert all(np.array_equal(a, b) for a, b in zip(got, one_group)), device
    assert np.array_equal(dx.cpu().numpy().view(np.uint64).reshape(xs.shape), xs)           # the caller's device rows are only read
    assert np.array_equal(dw.cpu().numpy().view(np.uint64).reshape(ws.shape), ws)


# ---- 7. end to end: inputs -> proofs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_end_to_end_mimc(gpu_ctx, curve):
    s = _mimc_key(gpu_ctx, curve)
    pm, pk, c, f = s["pm"], s["pk"], s["c"], s["f"]
    rows = _mimc_rows(c, 8, 8700)
    r_as = [[51 + i, 61 + i] for i in range(8)]
    limbs = [pm.partial_limbs(*p) for _, _, p in rows]
    proofs, statuses, instances = pm.prove_batch(pk, limbs, r_as, solve=True)
    assert statuses == [0] * 8 and instances == [inst for inst, _, _ in rows]          # [1, mimc_native]
    vk = pm.make_vk(pk, s["x"], s["z"])
    assert all(pm.verify(vk, inst[1:], p) for (inst, _, _), p in zip(rows, proofs))
    want, st = pm.prove_batch(pk, [(f.fr_limbs(inst), f.fr_limbs(wit)) for inst, wit, _ in rows], r_as)
    assert st == [0] * 8 and proofs == want                                            # the Python-synthesised assignments, same r_a
    t = pm.ctx.timings()
    assert t["witness_map"] > 0
    if curve == "bls12_381":
        # several groups (3, 3, 2) and device-resident partial assignments: the same bytes
        assert pk.n == 1 << 11 and 3 * (10 * pk.n + 22) <= 1 << 16 < 4 * (10 * pk.n + 22)
        gpu_ctx.set_option("msm_max_piece_log", 16)
        xs, ws = np.stack([p[0] for p in limbs]), np.stack([p[1] for p in limbs])
        dx, dw = torch.from_numpy(xs.view(np.int64)).cuda(), torch.from_numpy(ws.view(np.int64)).cuda()
        torch.cuda.synchronize()
        assert pm.prove_batch(pk, limbs, r_as, solve=True)[0] == want
        got = pm.prove_batch(pk, limbs, r_as, device_ptrs=(dx.data_ptr(), dw.data_ptr()), solve=True)
        assert got[0] == want and got[2] == instances


# ---- 8. without the flag nothing looks for markers; a proof in flight survives a solving check ---------------------------------------------------
def test_marker_without_the_flag(gpu_ctx):
    s = _diag_key(gpu_ctx, "bls12_381", 64)
    pm, pk = s["pm"], s["pk"]
    x, w = pm.partial_limbs([1], [3 + r for r in range(64)] * 2)
    w[64 + 10] = pm.partial_limbs([1], [None])[1][0]
    rc, n_bad, rows, _ = pk.r1cs_check(x, w, 4)
    assert (rc, n_bad, [int(v) for v in rows]) == (PM_OK, 1, [10, NONE, NONE, NONE])


def test_proof_in_flight_is_not_disturbed(gpu_ctx):
    s = _diag_key(gpu_ctx, "bls12_381", 257)
    pm, pk, f = s["pm"], s["pk"], s["f"]
    xl, wl = f.fr_limbs(s["inst"]), f.fr_limbs(s["wit"])
    partial = pm.partial_limbs([1], [5 + r for r in range(257)] + [None] * 257)
    r_a = [21, 34]
    want = pm.prove_native(pk, xl, wl, r_a)
    seen = []
    phase2, phase3 = pk.phase2, pk.phase3

    def solving(phase):
        def run(*args):                                       # a solving check between the phases of the proof in flight
            seen.append(pm.solve_batch(pk, [partial])[0])
            return phase(*args)
        return run
    pk.phase2, pk.phase3 = solving(phase2), solving(phase3)
    try:
        proof = pm.prove_limbs(pk, s["inst"], xl, wl, r_a)
    finally:
        del pk.phase2, pk.phase3
    assert seen == [(None, [1], [5 + r for r in range(257)] * 2)] * 2
    assert proof.to_bytes() == want
