"""GPU: PM_ASSIGNMENT_SOLVE on circuits that divide integers -- Euclidean division rows (csrc/solve.hip: solve_divrem, k_solve_divrem,
the division branch of k_solve_chain, the quotient marker in k_solve_pattern; csrc/divrem.cuh: the 256-bit division;
host/solve_plan.hpp: KIND_DIVREM).  The bar is equality, word for word, with Python integers: the generators' own assignments
(polymath_amd.circuits: DivRem, ModChain, native()) and divmod.

Shapes are the smallest at which each mechanism can differ.  DivRem with N pairs is ONE level of N divisions: N = 1 and 31 are walked
by the chain kernel, 32 is the first level with a k_solve_divrem launch of its own, 64 is a whole wave of it, 257 a 256-lane workgroup
and one lane; batches of 1, 3 and 70 are the chain kernel's partial wave and second workgroup and k_solve_divrem's grid y.  With
bits = 250 the operands reach every word of the division; a hand-written system without range checks takes them up to r - 1.
ModChain is 80 narrow levels: one chain launch that alternates ordinary steps and divisions, also with its rows reversed and shuffled."""
import numpy as np
import pytest
import torch        # noqa: F401  before libpolymath_hip.so is loaded: torch brings its own HIP runtime (tests/ntt_device_child.py)

from oracle.pyref.fields import CURVES
from witness_solve_helpers import BOTH, NONE, PM_ERR_INVALID_ARG, PM_OK, _completes, _rows, _setup, _solve, key_cache

pytestmark = pytest.mark.gpu

_cached = key_cache()


def _pairs(g, n, bits, i):
    """n (a, b) pairs of `bits`-bit operands, b >= 1, with the small edges among them; assignment i starts elsewhere in the list"""
    top = (1 << bits) - 1
    edges = [(0, 1), (top, 1), (top, top), (top - 1, top), (5, 9), (9, 9), (1 << (bits - 1), 3), (top, 2)]
    out = [edges[(i + j) % len(edges)] if j % 4 == 0 else (g.next_u64() & top, 1 + g.next_u64() % top) for j in range(n)]
    assert all(0 <= a <= top and 1 <= b <= top for a, b in out)
    return out


# ---- 1. DivRem: one level of N divisions, at the chain / level threshold and the wave and workgroup edges of k_solve_divrem ------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("n", [1, 31, 32, 64, 257])
def test_div_rem(gpu_ctx, curve, n):
    from polymath_amd import circuits as PC, polymath as PM
    r, bits = CURVES[curve].r, 16
    s = _cached((curve, "divrem", n), lambda: _setup(gpu_ctx, curve, PC.DivRem([(7, 3)] * n, bits), 12000 + n))
    q = s["q"]
    assert (q.m0, q.mw, q.nr) == (2, n * (4 + 3 * bits), n * (3 * bits + 4) + 1)
    partial = PC.DivRem([(7, 3)] * n, bits).partial(r)
    assert sum(v is PM.QUOTIENT for v in partial[1]) == n and sum(v is not None and v is not PM.QUOTIENT for v in partial[1]) == 2 * n
    g = PC.SplitMix64(12100 + n)
    for count in (1, 3, 70):
        circuits = [PC.DivRem(_pairs(g, n, bits, i), bits) for i in range(count)]
        assignments = [ci.native(r) for ci in circuits]
        inst, wit = assignments[0]
        assert inst[1] == sum(sum(divmod(a, b)) for a, b in circuits[0].pairs) and wit[2:4] == list(divmod(*circuits[0].pairs[0]))
        _completes(s, assignments, partial)


# ---- 2. wide operands: bits = 250, one level of 64 with the edge operands; and bare rows up to r - 1 -------------------------------------------
def _wide_pairs(g, bits, shift):
    top = (1 << bits) - 1
    pairs = [(a, d) for d in (1, top, 1 << 64, (1 << 192) + 1) for a in (0, d - 1, d, top)]
    while len(pairs) < 64:
        size = (30, 64, 65, 128, 191, 193, 250)[len(pairs) % 7]
        pairs.append((g.fr(1 << bits), 1 + g.fr(1 << size) % top))
    return pairs[shift:] + pairs[:shift]


@pytest.mark.parametrize("curve", BOTH)
def test_div_rem_wide_operands(gpu_ctx, curve):
    from polymath_amd import circuits as PC
    r, bits = CURVES[curve].r, 250
    s = _cached((curve, "divrem wide"), lambda: _setup(gpu_ctx, curve, PC.DivRem([(7, 3)] * 64, bits), 12200))
    partial = PC.DivRem([(7, 3)] * 64, bits).partial(r)
    g = PC.SplitMix64(12300)
    circuits = [PC.DivRem(_wide_pairs(g, bits, 5 * i), bits) for i in range(3)]
    assignments = [ci.native(r) for ci in circuits]
    for ci, (inst, wit) in zip(circuits, assignments):
        per = 4 + 3 * bits
        assert all(tuple(wit[j * per + 2:j * per + 4]) == divmod(a, d) for j, (a, d) in enumerate(ci.pairs))
    _completes(s, assignments[:1], partial)
    _completes(s, assignments, partial)


# columns: 0 one | 1 out (public) | per division a, d (given), q, rem.   Row i: q_i * d_i = a_i - rem_i, q in A for even i and in B for odd i,
# with coefficient 1 (i % 4 < 2) or 7 on q, on a and, negated, on rem;  last row: (sum q_i + rem_i) * 1 = out
def bare_system(r, n):
    from polymath_amd.polymath import R1CS
    a_rows, b_rows, c_rows, total = [], [], [], []
    for i in range(n):
        a, d, q, rem = (2 + 4 * i + k for k in range(4))
        cq = 1 if i % 4 < 2 else 7
        lone, known = [(cq, q)], [(1, d)]
        a_rows.append(lone if i % 2 == 0 else known)
        b_rows.append(known if i % 2 == 0 else lone)
        c_rows.append([(cq, a), (r - cq, rem)])
        total += [(1, q), (1, rem)]
    return R1CS(2, 4 * n, a_rows + [total], b_rows + [[(1, 0)]], c_rows + [[(1, 1)]])


def _bare_assignment(r, operands):
    wit, total = [], 0
    for a, d in operands:
        q, rem = divmod(a, d)
        wit += [a, d, q, rem]
        total += q + rem
    return [1, total % r], wit


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("n", [16, 40])
def test_bare_rows_up_to_the_modulus(gpu_ctx, curve, n):
    from polymath_amd import circuits as PC, polymath as PM
    r = CURVES[curve].r
    s = _cached((curve, "bare", n), lambda: _setup(gpu_ctx, curve, (bare_system(r, n),) + tuple(_bare_assignment(r, [(7, 3)] * n)), 12400 + n))
    edges = [(a, d) for d in (1, r - 1, 1 << 64, (1 << 192) + 1) for a in (0, d - 1, d, r - 1)]
    g = PC.SplitMix64(12500 + n)
    partial = ([1, None], [v for _ in range(n) for v in (0, 0, PM.QUOTIENT, None)])
    assignments = []
    for i in range(3):
        operands = [edges[(j + 5 * i) % 16] if j < 16 else (g.fr(r), 1 + g.fr(1 << (20, 70, 130, 200, 253)[j % 5]) % (r - 1)) for j in range(n)]
        assignments.append(_bare_assignment(r, operands))
    _completes(s, assignments, partial)


# ---- 3. d = 0 in one assignment of three: stuck at its division row, the neighbours complete ---------------------------------------------------
@pytest.mark.parametrize("curve,n", [("bls12_381", 32), ("bn254", 31)])
def test_zero_divisor_is_stuck(gpu_ctx, curve, n):
    from polymath_amd import circuits as PC
    r, bits = CURVES[curve].r, 16
    s = _cached((curve, "divrem", n), lambda: _setup(gpu_ctx, curve, PC.DivRem([(7, 3)] * n, bits), 12000 + n))
    pm, pk, q = s["pm"], s["pk"], s["q"]
    partial = PC.DivRem([(7, 3)] * n, bits).partial(r)
    g = PC.SplitMix64(12600)
    pairs = [_pairs(g, n, bits, i) for i in range(3)]
    pairs[1][5] = (1234, 0)
    assignments = [PC.DivRem(p, bits).native(r) for p in pairs]
    want, rows = _rows(s, assignments, partial)
    n_bad, bad_rows, stuck, full = _solve(s, rows)
    division_row = 5 * (3 * bits + 4) + 3 * bits
    assert stuck == [NONE, division_row, NONE] and n_bad == [0, NONE, 0]
    assert int(bad_rows[1][0]) == division_row and int(bad_rows[1][1]) == NONE
    assert np.array_equal(full[0], want[0]) and np.array_equal(full[2], want[2])
    limbs = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(3)]
    proofs, statuses, instances = pm.prove_batch(pk, limbs, [[31 + i, 41 + i] for i in range(3)], solve=True)
    assert statuses == [0, PM_ERR_INVALID_ARG, 0] and proofs[1] is None and instances == [assignments[0][0], None, assignments[2][0]]


# ---- 4. ModChain: 80 narrow levels, ordinary steps and divisions in turn, in one chain launch; reversed and shuffled --------------------------
def _mod_chain(g, steps):
    m = 2 + g.next_u64() % ((1 << 61) - 1)
    return dict(s0=g.next_u64() % m, g=g.next_u64(), c=g.next_u64(), m=m, steps=steps)


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("order", [None, "reverse", 8301])
def test_mod_chain(gpu_ctx, curve, order):
    from polymath_amd import circuits as PC
    r, steps = CURVES[curve].r, 40
    wrap = (lambda c: c) if order is None else (lambda c: PC.Reordered(c, order))
    s = _cached((curve, "modchain", order), lambda: _setup(gpu_ctx, curve, wrap(PC.ModChain(3, 5, 7, 11, steps)), 12700))
    q = s["q"]
    assert (q.m0, q.mw, q.nr) == (2, 4 + 3 * steps - 1, 2 * steps)
    partial = PC.ModChain(3, 5, 7, 11, steps).partial(r)
    g = PC.SplitMix64(12800)
    for count in (1, 70):
        assignments = []
        for i in range(count):
            kw = _mod_chain(g, steps)
            inst, wit = PC.ModChain(**kw).native(r)
            assert inst[1] == PC.mod_chain_native(**kw) and wit[:4] == [kw["s0"], kw["g"], kw["c"], kw["m"]]
            assignments.append((inst, wit))
        _completes(s, assignments, partial)


# ---- 5. inputs -> verified proofs: the same bytes as the same call on the completed assignment ---------------------------------------------------
@pytest.mark.parametrize("curve,which", [("bls12_381", "divrem"), ("bn254", "divrem"), ("bls12_381", "modchain"), ("bn254", "modchain")])
def test_inputs_to_proofs(gpu_ctx, curve, which):
    from polymath_amd import circuits as PC
    r, count = CURVES[curve].r, 3
    g = PC.SplitMix64(12900)
    if which == "divrem":
        s = _cached((curve, "divrem", 8), lambda: _setup(gpu_ctx, curve, PC.DivRem([(7, 3)] * 8, 16), 12008))
        circuits = [PC.DivRem(_pairs(g, 8, 16, i), 16) for i in range(count)]
    else:
        s = _cached((curve, "modchain", None), lambda: _setup(gpu_ctx, curve, PC.ModChain(3, 5, 7, 11, 40), 12700))
        circuits = [PC.ModChain(**_mod_chain(g, 40)) for i in range(count)]
    pm, pk, f, q = s["pm"], s["pk"], s["f"], s["q"]
    assignments = [ci.native(r) for ci in circuits]
    want, rows = _rows(s, assignments, circuits[0].partial(r))
    part = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(count)]
    full = [(np.ascontiguousarray(want[i, :q.m0]), np.ascontiguousarray(want[i, q.m0:])) for i in range(count)]
    r_as = [[51 + i, 61 + i] for i in range(count)]
    vk = pm.make_vk(pk, s["x"], s["z"])
    # pm_host_prove
    rc, solved = pk.host_prove("merlin", part[1][0], part[1][0], part[1][1], f.fr_limbs(r_as[1]), solve=True)
    rc2, plain = pk.host_prove("merlin", full[1][0], full[1][0], full[1][1], f.fr_limbs(r_as[1]))
    assert (rc, rc2) == (PM_OK, PM_OK) and solved == plain and pm.verify(vk, assignments[1][0][1:], solved)
    # pm_host_prove_batch, host glue and PM_PROVE_GLUE_DEVICE
    for glue in ("host", "device"):
        proofs, statuses, instances = pm.prove_batch(pk, part, r_as, solve=True, glue=glue)
        plain_proofs, plain_statuses = pm.prove_batch(pk, full, r_as, glue=glue)
        assert statuses == [0] * count and plain_statuses == [0] * count and instances == [inst for inst, _ in assignments], glue
        assert proofs == plain_proofs and proofs[1] == solved, glue
        assert all(pm.verify(vk, assignments[i][0][1:], proofs[i]) for i in range(count)), glue
    # from device pointers: the same bytes, and the caller's rows are only read
    xs, ws = np.ascontiguousarray(rows[:, :q.m0]), np.ascontiguousarray(rows[:, q.m0:])
    dx, dw = torch.from_numpy(xs.view(np.int64)).cuda(), torch.from_numpy(ws.view(np.int64)).cuda()
    torch.cuda.synchronize()
    got = pm.prove_batch(pk, part, r_as, device_ptrs=(dx.data_ptr(), dw.data_ptr()), solve=True)
    assert got[0] == proofs and got[2] == [inst for inst, _ in assignments]
    assert np.array_equal(dx.cpu().numpy().view(np.uint64).reshape(xs.shape), xs) and np.array_equal(dw.cpu().numpy().view(np.uint64).reshape(ws.shape), ws)


# ---- 6. the marker is explicit: mixed markers are a mismatch, the plain marker on q is today's refusal ----------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_markers_are_explicit(gpu_ctx, curve):
    from polymath_amd import circuits as PC
    r, n, bits = CURVES[curve].r, 8, 16
    s = _cached((curve, "divrem", n), lambda: _setup(gpu_ctx, curve, PC.DivRem([(7, 3)] * n, bits), 12008))
    pm, pk, q = s["pm"], s["pk"], s["q"]
    g = PC.SplitMix64(13000)
    circuits = [PC.DivRem(_pairs(g, n, bits, i), bits) for i in range(3)]
    assignments = [ci.native(r) for ci in circuits]
    partial = circuits[0].partial(r)
    per = 4 + 3 * bits
    q_cols = [q.m0 + j * per + 2 for j in range(n)]
    want, rows = _rows(s, assignments, partial)
    # assignment 2 marks the quotient of division 3 with the plain marker
    mixed = rows.copy()
    mixed[2, q_cols[3]] = (NONE,) * 4
    rc, n_bad, _, _ = pk.r1cs_check_batch(np.ascontiguousarray(mixed[:, :q.m0]), np.ascontiguousarray(mixed[:, q.m0:]), 2, solve=True)
    assert rc == PM_ERR_INVALID_ARG and "assignment 2 differs from assignment 0 at column %d" % q_cols[3] in pm.ctx.last_error(), pm.ctx.last_error()
    # every assignment marks every quotient with the plain marker (None): nothing is inferred, the row is refused as it always was
    plain = rows.copy()
    plain[:, q_cols] = (NONE,) * 4
    inst, wit = partial
    from polymath_amd import polymath as PM
    assert np.array_equal(np.concatenate(pm.partial_limbs(inst, [None if v is PM.QUOTIENT else v for v in wit])), plain[0])
    assert np.array_equal(np.concatenate(pm.partial_limbs(inst, wit)), rows[0])
    division_row = 3 * bits
    text = "row %d: two or more unknowns (columns %d and %d), and no is-zero pair: " % (division_row, q_cols[0], q_cols[0] + 1)
    for call in (lambda: pk.r1cs_check_batch(np.ascontiguousarray(plain[:, :q.m0]), np.ascontiguousarray(plain[:, q.m0:]), 2, solve=True)[0],
                 lambda: pk.host_prove("merlin", plain[0, :q.m0].copy(), plain[0, :q.m0].copy(), plain[0, q.m0:].copy(), s["f"].fr_limbs([3, 5]), solve=True)[0]):
        assert call() == PM_ERR_INVALID_ARG
        assert text in pm.ctx.last_error(), pm.ctx.last_error()
    # the refused pattern did not stay in the plan cache, and the context is as usable as before
    _completes(s, assignments, partial)
