"""GPU: PM_ASSIGNMENT_SOLVE on circuits whose rows are square linear systems in their unknowns -- linear blocks (csrc/solve.hip:
k_solve_block, the host inversion in solve_plan; csrc/solve_steps.cuh: solve_block_invert, solve_block_rhs, solve_block_out;
host/solve_plan.hpp: KIND_BLOCK).  The bar is equality, word for word, with Python integers: the generators' own assignments
(polymath_amd.circuits: LimbProduct, ProductChain, LinearBlocks, native()).

Shapes are the smallest at which each mechanism can differ.  k_solve_block gives a wave to a block and a lane to each of its k rows
and columns, four waves to a workgroup: LinearBlocks of m = 2, 3, 63, 64 are the lane-mask edges of one wave (one block, and five with
five inverses in the pool), m = 3 with 31, 32 and 257 blocks the workgroup edges (a last workgroup with three, four and one live
waves); batches of 1, 3 and 70 are grid y.  LimbProduct of l = 2, 4, 32 limbs (k = 3, 7, 63) with 40 products is 40 blocks through ONE
inverse, and with first = 0 an ordinary step in front of blocks of 2l - 2; ProductChain is block launches between chain launches.
Reordered: the same words with the rows reversed and shuffled.  On the code before linear blocks every solving call here is refused
with PM_ERR_INVALID_ARG ("two or more unknowns")."""
import numpy as np
import pytest
import torch        # noqa: F401  before libpolymath_hip.so is loaded: torch brings its own HIP runtime (tests/ntt_device_child.py)

from oracle.pyref.fields import CURVES
from witness_solve_helpers import BOTH, NONE, PM_ERR_INVALID_ARG, PM_OK, _completes, _rows, _setup, _solve, key_cache

pytestmark = pytest.mark.gpu

_cached = key_cache()


def _wrap(circuit, order):
    from polymath_amd import circuits as PC
    return circuit if order is None else PC.Reordered(circuit, order)


# ---- 1. LinearBlocks: the lane-mask edges of a wave, the workgroup edges, grid y ------------------------------------------------------------------
def _blocks_key(gpu_ctx, curve, m, count, order=None):
    from polymath_amd import circuits as PC
    return _cached((curve, "blocks", m, count, order), lambda: _setup(gpu_ctx, curve, _wrap(PC.LinearBlocks(m, count, 17000 + m), order), 17100 + m + count))


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("m,count", [(2, 1), (2, 5), (3, 1), (3, 5), (63, 1), (63, 5), (64, 1), (64, 5), (3, 31), (3, 32), (3, 257)])
def test_linear_blocks(gpu_ctx, curve, m, count):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    s = _blocks_key(gpu_ctx, curve, m, count)
    q = s["q"]
    assert (q.m0, q.mw, q.nr) == (2, count * (3 * m + 1), count * (m + 1) + 1)
    partial = PC.LinearBlocks(m, count, 17000 + m).partial(r)
    assert sum(v is None for v in partial[1]) == count * (m + 1)
    for batch in (1, 3, 70):
        circuits = [PC.LinearBlocks(m, count, 17000 + m, values=17200 + 100 * batch + i) for i in range(batch)]
        assignments = [ci.native(r) for ci in circuits]
        assert assignments[0] != assignments[-1] or batch == 1
        _completes(s, assignments, partial)


# ---- 2. LimbProduct: 40 products through one inverse; the point 0 as an ordinary step in front of the blocks -----------------------------------------
def _product_key(gpu_ctx, curve, limbs, count, first, order=None):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    return _cached((curve, "product", limbs, count, first, order),
                   lambda: _setup(gpu_ctx, curve, _wrap(PC.LimbProduct(PC.limb_products(r, count, limbs, 17300), first), order), 17300 + limbs + first))


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("limbs,first", [(2, 1), (4, 1), (32, 1), (4, 0)])
def test_limb_product(gpu_ctx, curve, limbs, first):
    from polymath_amd import circuits as PC
    r, count = CURVES[curve].r, 40
    s = _product_key(gpu_ctx, curve, limbs, count, first)
    q = s["q"]
    assert (q.m0, q.mw, q.nr) == (2, count * (4 * limbs), count * (2 * limbs) + 1)
    partial = PC.LimbProduct(PC.limb_products(r, count, limbs, 17300), first).partial(r)
    assert sum(v is None for v in partial[1]) == count * 2 * limbs
    # the batch is grid y whatever k is: the wide products run the small batch only
    for batch in ((3,) if limbs == 32 else (1, 3, 70)):
        circuits = [PC.LimbProduct(PC.limb_products(r, count, limbs, 17400 + 100 * batch + i), first) for i in range(batch)]
        assignments = [ci.native(r) for ci in circuits]
        inst, wit = assignments[0]
        a, b = circuits[0].products[7]
        at = 7 * 4 * limbs + 2 * limbs
        assert wit[at:at + 2 * limbs - 1] == PC.limb_product(a, b, r) and wit[at + 2 * limbs - 1] == sum(PC.limb_product(a, b, r)) % r
        _completes(s, assignments, partial)


# ---- 3. ProductChain: block launches between chain launches ---------------------------------------------------------------------------------------------
def _chain_key(gpu_ctx, curve, order=None):
    from polymath_amd import circuits as PC
    return _cached((curve, "chain", order), lambda: _setup(gpu_ctx, curve, _wrap(PC.ProductChain([1, 2, 3], [4, 5, 6], 5), order), 17500))


def _chains(curve, batch, seed):
    from polymath_amd import circuits as PC
    r, g = CURVES[curve].r, PC.SplitMix64(seed)
    return [PC.ProductChain([g.fr(r) for _ in range(3)], [g.fr(r) for _ in range(3)], 5) for _ in range(batch)]


@pytest.mark.parametrize("curve", BOTH)
def test_product_chain(gpu_ctx, curve):
    r = CURVES[curve].r
    s = _chain_key(gpu_ctx, curve)
    q = s["q"]
    assert (q.m0, q.mw, q.nr) == (2, 6 + 5 * 6, 5 * 6 + 1)
    circuits = _chains(curve, 70, 17600)
    _completes(s, [ci.native(r) for ci in circuits], circuits[0].partial(r))


# ---- 4. Reordered: the same words in any row order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("order", ["reverse", 17701, 17702])
def test_reordered(gpu_ctx, curve, order):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    chains = _chains(curve, 3, 17700)
    products = [PC.LimbProduct(PC.limb_products(r, 8, 4, 17710 + i)) for i in range(3)]
    from_zero = [PC.LimbProduct(PC.limb_products(r, 8, 4, 17720 + i), 0) for i in range(3)]
    blocks = [PC.LinearBlocks(3, 5, 17003, values=17730 + i) for i in range(3)]
    for circuits, key in ((chains, lambda o: _chain_key(gpu_ctx, curve, o)), (products, lambda o: _product_key(gpu_ctx, curve, 4, 8, 1, o)),
                          (from_zero, lambda o: _product_key(gpu_ctx, curve, 4, 8, 0, o)), (blocks, lambda o: _blocks_key(gpu_ctx, curve, 3, 5, o))):
        assignments, partial = [ci.native(r) for ci in circuits], circuits[0].partial(r)
        assert np.array_equal(_completes(key(order), assignments, partial), _completes(key(None), assignments, partial))


# ---- 5. through the C ABI: a singular block, 65 unknowns, k - 1 rows ------------------------------------------------------------------------------------
# columns: 0 one | 1 x (public, given) | then the given g_i, then the unknown u_j.  rows: g_i * 1 = sum_j M_ij u_j, and x * 1 = g_0 (a check row)
def _system(r, mat):
    from polymath_amd.polymath import R1CS
    k, n = len(mat[0]), len(mat)
    a = [[(1, 2 + i)] for i in range(n)] + [[(1, 1)]]
    b = [[(1, 0)]] * (n + 1)
    c = [[(coef % r, 2 + n + j) for j, coef in enumerate(row) if coef % r] for row in mat] + [[(1, 2)]]
    return R1CS(2, n + k, a, b, c), [1, 5], [5] + [0] * (n - 1) + [0] * k


def _refused(s, k, n):
    """the check call on one assignment with the k columns after the n given ones unknown -> (rc, message); the caller's rows stay as they are"""
    from polymath_amd import api
    q = s["q"]
    xs, ws = s["f"].fr_limbs([1, 5]).reshape(1, 2, 4), s["f"].fr_limbs([5] + [0] * (n - 1 + k)).reshape(1, n + k, 4)
    ws[:, n:] = api.UNKNOWN_LIMBS
    xs, ws = np.ascontiguousarray(xs), np.ascontiguousarray(ws)
    before = (xs.copy(), ws.copy())
    assert ws.shape[1] == q.mw
    rc = s["pk"].r1cs_check_batch(xs, ws, 2, solve=True)[0]
    assert np.array_equal(xs, before[0]) and np.array_equal(ws, before[1])
    return rc, s["pm"].ctx.last_error()


@pytest.mark.parametrize("curve", BOTH)
def test_refusals(gpu_ctx, curve):
    r = CURVES[curve].r
    # rows 0 and 1 are sound over (u_0, u_1) ... but rows 2 and 3 over (u_2, u_3) are proportional
    mat = [[1, 1, 0, 0], [1, 2, 0, 0], [0, 0, 1, 3], [0, 0, 2, 6]]
    s = _cached((curve, "singular"), lambda: _setup(gpu_ctx, curve, _system(r, mat), 17800))
    rc, message = _refused(s, 4, 4)
    assert rc == PM_ERR_INVALID_ARG and "pm solve: rows 2, 3: the linear block over columns 8, 9 is singular (no pivot in column 9)" in message, message
    # 65 unknowns in 65 rows
    wide = [[pow(i + 1, j, r) for j in range(65)] for i in range(65)]
    s = _cached((curve, "wide"), lambda: _setup(gpu_ctx, curve, _system(r, wide), 17801))
    rc, message = _refused(s, 65, 65)
    assert rc == PM_ERR_INVALID_ARG and "row 0: two or more unknowns (columns 67 and 68)" in message, message
    assert message.endswith("; in any row order: column 67 stays unknown, and no linear block: 65 unknowns exceed 64"), message
    # k - 1 rows: refused as before
    short = [[1, 1, 1], [1, 2, 4]]
    s = _cached((curve, "short"), lambda: _setup(gpu_ctx, curve, _system(r, short), 17802))
    rc, message = _refused(s, 3, 2)
    assert rc == PM_ERR_INVALID_ARG and "row 0: two or more unknowns (columns 4 and 5)" in message and message.endswith("; in any row order: column 4 stays unknown"), message
    # ... and with the third row it completes: the refusals left nothing behind
    full = [[1, 1, 1], [1, 2, 4], [1, 3, 9]]
    s = _cached((curve, "full"), lambda: _setup(gpu_ctx, curve, _system(r, full), 17803))
    u = [7, r - 2, 11]
    g = [sum(c * v for c, v in zip(row, u)) % r for row in full]
    _completes(s, [([1, g[0]], g + u)], ([1, g[0]], g + [None] * 3))


# ---- 6. inputs -> verified proofs: the same bytes as the same call on the Python-completed assignment ---------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_inputs_to_proofs(gpu_ctx, curve):
    from polymath_amd import circuits as PC
    r, count = CURVES[curve].r, 5
    s = _product_key(gpu_ctx, curve, 4, 8, 1)
    pm, pk, f, q = s["pm"], s["pk"], s["f"], s["q"]
    circuits = [PC.LimbProduct(PC.limb_products(r, 8, 4, 17900 + i)) for i in range(count)]
    assignments = [ci.native(r) for ci in circuits]
    want, rows = _rows(s, assignments, circuits[0].partial(r))
    part = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(count)]
    full = [(np.ascontiguousarray(want[i, :q.m0]), np.ascontiguousarray(want[i, q.m0:])) for i in range(count)]
    r_as = [[51 + i, 61 + i] for i in range(count)]
    vk = pm.make_vk(pk, s["x"], s["z"])
    # pm_host_prove, one row
    rc, solved = pk.host_prove("merlin", part[1][0], part[1][0], part[1][1], f.fr_limbs(r_as[1]), solve=True)
    rc2, plain = pk.host_prove("merlin", full[1][0], full[1][0], full[1][1], f.fr_limbs(r_as[1]))
    assert (rc, rc2) == (PM_OK, PM_OK) and solved == plain and pm.verify(vk, assignments[1][0][1:], solved)
    # pm_host_prove_batch, host glue and PM_PROVE_GLUE_DEVICE
    proofs = None
    for glue in ("host", "device"):
        proofs, statuses, instances = pm.prove_batch(pk, part, r_as, solve=True, glue=glue)
        plain_proofs, plain_statuses = pm.prove_batch(pk, full, r_as, glue=glue)
        assert statuses == [0] * count and plain_statuses == [0] * count and instances == [inst for inst, _ in assignments], glue
        assert proofs == plain_proofs and proofs[1] == solved, glue
        assert all(pm.verify(vk, assignments[i][0][1:], proofs[i]) for i in range(count)), glue
    # check_batch: no failing row
    assert pm.check_batch(pk, part, solve=True) == [(0, [])] * count
    assert pm.solve_batch(pk, part) == [(None, inst, wit) for inst, wit in assignments]
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


# ---- 7. a wrong given limb: the block never sticks -- the assignment completes to the product of the limbs as given, and proves ----------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_wrong_limb_still_completes(gpu_ctx, curve):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    s = _product_key(gpu_ctx, curve, 4, 8, 1)
    pm, pk, q = s["pm"], s["pk"], s["q"]
    products = PC.limb_products(r, 8, 4, 17950)
    meant = PC.LimbProduct(products).native(r)
    products[3][0][2] = 0                     # a limb the caller did not mean: zero, and r - 1
    products[5][1][0] = r - 1
    given = PC.LimbProduct(products)
    got = given.native(r)
    assert got != meant
    want, rows = _rows(s, [got, meant], given.partial(r))
    n_bad, _, stuck, full = _solve(s, rows)
    assert n_bad == [0, 0] and stuck == [NONE, NONE] and np.array_equal(full, want)
    part = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(2)]
    proofs, statuses, instances = pm.prove_batch(pk, part, [[71, 72], [73, 74]], solve=True)
    tap_stuck, _ = pk.solve_results(2)                                    # tap 9
    assert [int(v) for v in tap_stuck] == [NONE, NONE] and statuses == [0, 0] and instances == [got[0], meant[0]]
    vk = pm.make_vk(pk, s["x"], s["z"])
    assert pm.verify(vk, got[0][1:], proofs[0]) and pm.verify(vk, meant[0][1:], proofs[1]) and not pm.verify(vk, meant[0][1:], proofs[0])
