"""GPU: PM_ASSIGNMENT_SOLVE on circuits that take square roots -- square-root rows (csrc/solve.hip: k_solve_sqrt, the square-root branch
of k_solve_chain<P, true>, the square-root marker in k_solve_pattern; csrc/solve_steps.cuh: solve_sqrt; csrc/sqrt.cuh: fr_sqrt;
csrc/divrem.cuh: marker_byte; host/solve_plan.hpp: KIND_SQRT).  The bar is equality, word for word, with Python integers: the
generators' own assignments (polymath_amd.circuits: SquareRoots, EdwardsDecompress, native(); polymath.small_sqrt).

Shapes are the smallest at which each mechanism can differ.  SquareRoots of width W is ONE level of W square-root rows: W = 1 and 31
are walked by the chain kernel, 32 is the first level with a k_solve_sqrt launch of its own, 64 is a whole wave of it, 257 a 256-lane
workgroup and one lane; batches of 1, 3 and 70 are the chain kernel's partial wave and second workgroup and k_solve_sqrt's grid y.
The operands are random squares and the edge list of the CPU self-test: 0, 1, 4, r - 1 and, for every j = 0 .. s, the square of an
element whose 2-power part has order 2^j (every iteration of the root routine's loop nest takes both sides of its select).
EdwardsDecompress of 3 points is one dividing chain launch (the root feeds a product and a decomposition of bitlength(r) - 1 bits);
of 33 points every level is a wide launch: ordinary steps, dividing steps, k_solve_sqrt, decompositions.  Both also with their rows
reversed and shuffled."""
import numpy as np
import pytest
import torch        # noqa: F401  before libpolymath_hip.so is loaded: torch brings its own HIP runtime (tests/ntt_device_child.py)

from oracle.pyref.fields import CURVES
from witness_solve_helpers import BOTH, NONE, PM_ERR_INVALID_ARG, PM_OK, _rows, _setup, _solve, key_cache

pytestmark = pytest.mark.gpu

_cached = key_cache()
GENERATOR = {"bls12_381": (7, 32), "bn254": (5, 28)}      # the multiplicative generator and the 2-adicity of r - 1


def _rows4(s, assignments, partial):
    """witness_solve_helpers._rows with the fourth marker: PM.SQRT in `partial` becomes api.SQRT_LIMBS"""
    from polymath_amd import api, polymath as PM
    plain = tuple([None if v is PM.SQRT else v for v in part] for part in partial)
    want, rows = _rows(s, assignments, plain)
    rows[:, np.array([v is PM.SQRT for v in list(partial[0]) + list(partial[1])], dtype=bool)] = api.SQRT_LIMBS
    return want, rows


def _completes(s, assignments, partial):
    want, rows = _rows4(s, assignments, partial)
    n_bad, _, stuck, full = _solve(s, rows)
    count = len(assignments)
    assert n_bad == [0] * count and stuck == [NONE] * count, (count, n_bad, stuck)
    assert np.array_equal(full, want), count
    return full


def _edge_squares(curve):
    """0, 1, 4, r - 1 and, for j = 0 .. s, y^2 with y = ROOT^(2^(s - j)) h, ROOT = g^((r - 1) / 2^s), h = 3^(2^s) of odd order"""
    r = CURVES[curve].r
    g, s = GENERATOR[curve]
    root, h = pow(g, (r - 1) >> s, r), pow(3, 1 << s, r)
    return [0, 1, 4, r - 1] + [pow(pow(root, 1 << (s - j), r) * h % r, 2, r) for j in range(s + 1)]


_EDGE = {}


def _squares(curve, g, width, shift):
    """`width` squares: the edge list from position `shift` on, random squares between its entries"""
    return [c for c, _ in _squares_and_roots(curve, g, width, shift)]


def _squares_and_roots(curve, g, width, shift):
    """_squares as (c, the smaller root of c): the edge list's roots are computed once per curve, a random square's root is known"""
    r = CURVES[curve].r
    if curve not in _EDGE:
        _EDGE[curve] = [(c, _small(r, c)) for c in _edge_squares(curve)]
    edge, out = _EDGE[curve], []
    for i in range(width):
        y = g.fr(r) if i % 2 else None
        out.append(edge[(i // 2 + shift) % len(edge)] if y is None else (y * y % r, min(y, r - y)))
    return out


def _assignment(r, pairs):
    """SquareRoots(...).native(r) from (c, root) pairs"""
    return [1, sum(u for _, u in pairs) % r], [v for pair in pairs for v in pair]


def _roots_key(gpu_ctx, curve, width):
    from polymath_amd import circuits as PC
    return _cached((curve, "roots", width), lambda: _setup(gpu_ctx, curve, PC.SquareRoots([4] * width), 15000 + width))


# ---- 1. SquareRoots: one level of W square-root rows, at the chain / level threshold and the wave and workgroup edges of k_solve_sqrt ----------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("width", [1, 31, 32, 64, 257])
def test_square_roots(gpu_ctx, curve, width):
    from polymath_amd import circuits as PC, polymath as PM
    r = CURVES[curve].r
    s = _roots_key(gpu_ctx, curve, width)
    q = s["q"]
    assert (q.m0, q.mw, q.nr) == (2, 2 * width, width + 1)
    partial = PC.SquareRoots([4] * width).partial(r)
    assert partial == ([1, None], [4, PM.SQRT] * width)
    g = PC.SplitMix64(15100 + width)
    for count in (1, 3, 70):
        pairs = [_squares_and_roots(curve, g, width, 7 * i + count) for i in range(count)]
        assignments = [_assignment(r, p) for p in pairs]
        assert PC.SquareRoots([c for c, _ in pairs[0]]).native(r) == assignments[0]
        for inst, wit in assignments:
            assert all(u <= (r - 1) // 2 and u * u % r == c for c, u in zip(wit[0::2], wit[1::2])) and inst[1] == sum(wit[1::2]) % r
        _completes(s, assignments, partial)


# ---- 2. a non-residue in some assignments of a batch: stuck at its own row, the neighbours complete ------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("width", [31, 32])
def test_non_residue_is_stuck(gpu_ctx, curve, width):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    s = _roots_key(gpu_ctx, curve, width)
    pm, pk, q = s["pm"], s["pk"], s["q"]
    partial = PC.SquareRoots([4] * width).partial(r)
    g = PC.SplitMix64(15200 + width)
    values = [_squares(curve, g, width, i) for i in range(5)]
    generator = GENERATOR[curve][0]
    values[1][5] = generator                                                 # row i is the square-root row of value i
    values[3][width - 1] = generator * 4 % r
    values[3][9] = generator                                                 # two in one assignment: the smaller row is reported
    assert _small(r, generator) is None and _small(r, generator * 4 % r) is None
    assignments = [PC.SquareRoots(v).native(r) for v in values]
    want, rows = _rows4(s, assignments, partial)
    n_bad, bad_rows, stuck, full = _solve(s, rows)
    assert stuck == [NONE, 5, NONE, 9, NONE] and n_bad == [0, NONE, 0, NONE, 0]
    assert [int(bad_rows[i][0]) for i in (1, 3)] == [5, 9] and int(bad_rows[1][1]) == NONE
    for i in (0, 2, 4):
        assert np.array_equal(full[i], want[i]), i
    limbs = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(5)]
    for glue in ("host", "device"):
        proofs, statuses, instances = pm.prove_batch(pk, limbs, [[31 + i, 41 + i] for i in range(5)], solve=True, glue=glue)
        assert statuses == [0, PM_ERR_INVALID_ARG, 0, PM_ERR_INVALID_ARG, 0] and proofs[1] is None and proofs[3] is None, glue
        assert instances == [assignments[0][0], None, assignments[2][0], None, assignments[4][0]], glue
    vk = pm.make_vk(pk, s["x"], s["z"])
    assert all(pm.verify(vk, assignments[i][0][1:], proofs[i]) for i in (0, 2, 4))


def _small(r, c):
    from polymath_amd import polymath as PM
    return PM.small_sqrt(r, c)


# ---- 3. EdwardsDecompress: the root behind a division and in front of a product and a decomposition; chain and wide; in order, reversed, shuffled ----
def _decompress_key(gpu_ctx, curve, points, order):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    wrap = (lambda c: c) if order is None else (lambda c: PC.Reordered(c, order))
    return _cached((curve, "decompress", points, order), lambda: _setup(gpu_ctx, curve, wrap(PC.EdwardsDecompress(PC.edwards_ys(r, points, 15300), [0] * points)), 15300 + points))


def _points(curve, points, count, seed):
    """per assignment (ys, signs): fresh ordinates of curve points, every sign pattern"""
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    ys = PC.edwards_ys(r, points * count, seed)
    return [(ys[i * points:(i + 1) * points], [(i + j) % 2 for j in range(points)]) for i in range(count)]


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("points", [3, 33])
@pytest.mark.parametrize("order", [None, "reverse", 9203])
def test_edwards_decompress(gpu_ctx, curve, points, order):
    from polymath_amd import circuits as PC, polymath as PM
    r = CURVES[curve].r
    s = _decompress_key(gpu_ctx, curve, points, order)
    q = s["q"]
    nb = r.bit_length() - 1
    assert (q.m0, q.mw, q.nr) == (2, points * (6 + nb), points * (6 + nb) + 1)
    partial = PC.EdwardsDecompress([2] * points, [0] * points).partial(r)
    assert sum(v is PM.SQRT for v in partial[1]) == points and sum(v is not None and v is not PM.SQRT for v in partial[1]) == 2 * points
    for count in ((1, 70) if order is None and points == 3 else (3,)):
        inputs = _points(curve, points, count, 15400 + count)
        assignments = [PC.EdwardsDecompress(ys, signs).native(r) for ys, signs in inputs]
        full = _completes(s, assignments, partial)
        if order is not None:      # the same words as the circuit in its own row order gives
            assert np.array_equal(_completes(_decompress_key(gpu_ctx, curve, points, None), assignments, partial), full)


# ---- 4. inputs -> verified proofs: the same bytes as the same call on the Python-completed assignment -------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_inputs_to_proofs(gpu_ctx, curve):
    from polymath_amd import api, circuits as PC
    r, count, points = CURVES[curve].r, 5, 3
    s = _decompress_key(gpu_ctx, curve, points, None)
    pm, pk, f, q = s["pm"], s["pk"], s["f"], s["q"]
    circuits = [PC.EdwardsDecompress(ys, signs) for ys, signs in _points(curve, points, count, 15500)]
    assignments = [ci.native(r) for ci in circuits]
    want, rows = _rows4(s, assignments, circuits[0].partial(r))
    part = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(count)]
    full = [(np.ascontiguousarray(want[i, :q.m0]), np.ascontiguousarray(want[i, q.m0:])) for i in range(count)]
    r_as = [[51 + i, 61 + i] for i in range(count)]
    vk = pm.make_vk(pk, s["x"], s["z"])
    # pm_host_prove
    rc, solved = pk.host_prove("merlin", part[1][0], part[1][0], part[1][1], f.fr_limbs(r_as[1]), solve=True)
    rc2, plain = pk.host_prove("merlin", full[1][0], full[1][0], full[1][1], f.fr_limbs(r_as[1]))
    assert (rc, rc2) == (PM_OK, PM_OK) and solved == plain and pm.verify(vk, assignments[1][0][1:], solved)
    # pm_host_prove_batch, host glue and PM_PROVE_GLUE_DEVICE; tap 11 of the device mode against the challenges of the host mode's proofs
    proofs = None
    for glue in ("host", "device"):
        proofs, statuses, instances = pm.prove_batch(pk, part, r_as, solve=True, glue=glue)
        tap = pk.glue_challenges(count).copy() if glue == "device" else None
        plain_proofs, plain_statuses = pm.prove_batch(pk, full, r_as, glue=glue)
        assert statuses == [0] * count and plain_statuses == [0] * count and instances == [inst for inst, _ in assignments], glue
        assert proofs == plain_proofs and proofs[1] == solved, glue
        assert all(pm.verify(vk, assignments[i][0][1:], proofs[i]) for i in range(count)), glue
    host_proofs = pm.prove_batch(pk, part, r_as, solve=True, glue="host")[0]
    pub = np.stack([f.fr_limbs(inst[1:]) for inst, _ in assignments])
    x1, x2, c_at, ok = api.verifier_challenges_batch(gpu_ctx, curve, "merlin", vk, pub, host_proofs)
    assert ok.tolist() == [1] * count and np.array_equal(tap[:, 0], x1) and np.array_equal(tap[:, 1], x2) and np.array_equal(tap[:, 3], c_at)
    # several groups, host and device pointers: the same words and the same bytes, and the caller's rows are only read
    xs, ws = np.ascontiguousarray(rows[:, :q.m0]), np.ascontiguousarray(rows[:, q.m0:])
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
    for glue in ("host", "device"):
        assert pm.prove_batch(pk, part, r_as, solve=True, glue=glue)[0] == proofs, glue
        got = pm.prove_batch(pk, part, r_as, device_ptrs=(dx.data_ptr(), dw.data_ptr()), solve=True, glue=glue)
        assert got[0] == proofs and got[2] == [inst for inst, _ in assignments], glue
    assert np.array_equal(dx.cpu().numpy().view(np.uint64).reshape(xs.shape), xs) and np.array_equal(dw.cpu().numpy().view(np.uint64).reshape(ws.shape), ws)


# ---- 5. a square-root column that is a public input: the hashed instance carries the solved value under both glue modes ---------------------------
# columns: 0 one | 1 u (public, the root) | 2 c, 3 w (given), 4 cw.   row 0: u * u = c      row 1: c * w = cw (a check row)
def public_system(r):
    from polymath_amd.polymath import R1CS
    return R1CS(2, 3, [[(1, 1)], [(1, 2)]], [[(1, 1)], [(1, 3)]], [[(1, 2)], [(1, 4)]])


@pytest.mark.parametrize("curve", BOTH)
def test_root_as_public_input(gpu_ctx, curve):
    from polymath_amd import api, polymath as PM
    r = CURVES[curve].r
    s = _cached((curve, "public"), lambda: _setup(gpu_ctx, curve, (public_system(r), [1, 2], [4, 5, 20]), 15600))
    pm, pk, f, q = s["pm"], s["pk"], s["f"], s["q"]
    squares = [4, 0, r - 1, pow(r - 3, 2, r), _edge_squares(curve)[-1]]
    count = len(squares)
    assignments = [([1, PM.small_sqrt(r, c)], [c, 5, 5 * c % r]) for c in squares]
    assert [inst[1] for inst, _ in assignments[:2]] == [2, 0] and assignments[3][0][1] == 3
    want, rows = _rows4(s, assignments, ([1, PM.SQRT], [0, 0, 0]))
    assert tuple(int(v) for v in rows[0, 1]) == api.SQRT_LIMBS
    part = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(count)]
    full = [(np.ascontiguousarray(want[i, :q.m0]), np.ascontiguousarray(want[i, q.m0:])) for i in range(count)]
    r_as = [[71 + i, 81 + i] for i in range(count)]
    vk = pm.make_vk(pk, s["x"], s["z"])
    for glue in ("host", "device"):
        proofs, statuses, instances = pm.prove_batch(pk, part, r_as, solve=True, glue=glue)
        stuck, inst = pk.solve_results(count)                                                        # tap 9: the completed instance
        assert [int(v) for v in stuck] == [NONE] * count and np.array_equal(inst, want[:, :q.m0]), glue
        assert statuses == [0] * count and instances == [inst for inst, _ in assignments], glue
        assert proofs == pm.prove_batch(pk, full, r_as, glue=glue)[0], glue
        assert all(pm.verify(vk, assignments[i][0][1:], proofs[i]) for i in range(count)), glue
        assert not pm.verify(vk, [r - assignments[0][0][1]], proofs[0]), glue                        # the value that was hashed is the SMALLER root
    rc, one = pk.host_prove("merlin", part[3][0], part[3][0], part[3][1], f.fr_limbs(r_as[3]), solve=True)
    assert rc == PM_OK and one == proofs[3]


# ---- 6. the marker is explicit: the plain marker is refused as it always was, mixed markers are a mismatch ------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_plain_marker_is_refused(gpu_ctx, curve):
    from polymath_amd import circuits as PC, polymath as PM
    r, width = CURVES[curve].r, 31
    s = _roots_key(gpu_ctx, curve, width)
    pm, pk, q = s["pm"], s["pk"], s["q"]
    g = PC.SplitMix64(15700)
    circuits = [PC.SquareRoots(_squares(curve, g, width, i)) for i in range(3)]
    assignments = [ci.native(r) for ci in circuits]
    partial = circuits[0].partial(r)
    want, rows = _rows4(s, assignments, partial)
    inst, wit = partial
    plain = rows.copy()
    plain[:, [q.m0 + 2 * i + 1 for i in range(width)]] = (NONE,) * 4
    assert np.array_equal(np.concatenate(pm.partial_limbs(inst, [None if v is PM.SQRT else v for v in wit])), plain[0])
    assert np.array_equal(np.concatenate(pm.partial_limbs(inst, wit)), rows[0])
    text = "row 0: unknown column %d occurs in A and in B" % (q.m0 + 1)
    part = [(np.ascontiguousarray(plain[i, :q.m0]), np.ascontiguousarray(plain[i, q.m0:])) for i in range(3)]

    def batch_prove():
        try:
            pm.prove_batch(pk, part, [[3, 5]] * 3, solve=True)
        except Exception:
            return PM_ERR_INVALID_ARG
        return PM_OK
    for call in (lambda: pk.r1cs_check_batch(np.ascontiguousarray(plain[:, :q.m0]), np.ascontiguousarray(plain[:, q.m0:]), 2, solve=True)[0],
                 lambda: pk.host_prove("merlin", part[0][0].copy(), part[0][0].copy(), part[0][1].copy(), s["f"].fr_limbs([3, 5]), solve=True)[0],
                 batch_prove):
        assert call() == PM_ERR_INVALID_ARG
        assert text in pm.ctx.last_error(), pm.ctx.last_error()
    # the refused pattern did not stay in the plan cache, and the context is as usable as before
    _completes(s, assignments, partial)


@pytest.mark.parametrize("curve", BOTH)
def test_mixed_markers_are_a_mismatch(gpu_ctx, curve):
    from polymath_amd import api, circuits as PC
    r, width = CURVES[curve].r, 31
    s = _roots_key(gpu_ctx, curve, width)
    pm, pk, q = s["pm"], s["pk"], s["q"]
    g = PC.SplitMix64(15800)
    assignments = [PC.SquareRoots(_squares(curve, g, width, i)).native(r) for i in range(3)]
    partial = PC.SquareRoots([4] * width).partial(r)
    want, rows = _rows4(s, assignments, partial)
    column = q.m0 + 2 * 12 + 1
    for other, who in (((NONE,) * 4, 1), (api.QUOTIENT_LIMBS, 2), (api.INDICATOR_LIMBS, 1)):
        mixed = rows.copy()
        mixed[who, column] = other                                           # one assignment marks u_12 with another marker
        rc, n_bad, bad_rows, _ = pk.r1cs_check_batch(np.ascontiguousarray(mixed[:, :q.m0]), np.ascontiguousarray(mixed[:, q.m0:]), 2, solve=True)
        assert rc == PM_ERR_INVALID_ARG and "assignment %d differs from assignment 0 at column %d" % (who, column) in pm.ctx.last_error(), pm.ctx.last_error()
    # the reverse: assignment 0 marks it plainly and assignment 1 with the square-root marker
    mixed = rows.copy()
    mixed[0, column] = (NONE,) * 4
    mixed[2, column] = (NONE,) * 4
    part = [(np.ascontiguousarray(mixed[i, :q.m0]), np.ascontiguousarray(mixed[i, q.m0:])) for i in range(3)]
    with pytest.raises(Exception):
        pm.prove_batch(pk, part, [[3, 5]] * 3, solve=True)
    assert "assignment 1 differs from assignment 0 at column %d" % column in pm.ctx.last_error()
    # the refused batches left nothing behind: the context is as usable as before
    _completes(s, assignments, partial)
