"""GPU: PM_ASSIGNMENT_SOLVE on circuits that read a table at a signal -- indicator rows (csrc/solve.hip: solve_indicator,
k_solve_indicator, the indicator branch of both k_solve_chain instantiations, the indicator marker in k_solve_pattern; csrc/divrem.cuh:
marker_byte, indicator_of; host/solve_plan.hpp: KIND_INDICATOR).  The bar is equality, word for word, with Python integers: the
generators' own assignments (polymath_amd.circuits: Decoder, TableWalk, native()).

Shapes are the smallest at which each mechanism can differ.  Decoder of width W is ONE level of W indicator rows: W = 1 and 31 are
walked by the chain kernel, 32 is the first level with a k_solve_indicator launch of its own, 64 is a whole wave of it, 257 a 256-lane
workgroup and one lane; batches of 1, 3 and 70 are the chain kernel's partial wave and second workgroup and k_solve_indicator's grid y.
The hit is first, last, in the middle and absent (index = width, index = r - 1) and differs per assignment.  TableWalk at width 8 and
40 steps is one chain launch (120 narrow levels with signals, 80 with constants; neither divides), at width 40 and 6 steps wide
launches of indicators and of ordinary steps in turn; both also with their rows reversed and shuffled."""
import numpy as np
import pytest
import torch        # noqa: F401  before libpolymath_hip.so is loaded: torch brings its own HIP runtime (tests/ntt_device_child.py)

from oracle.pyref.fields import CURVES
from witness_solve_helpers import BOTH, NONE, PM_ERR_INVALID_ARG, PM_OK, _completes, _rows, _setup, _solve, key_cache

pytestmark = pytest.mark.gpu

_cached = key_cache()


def _indices(width, r, count, shift):
    """the hit first, last, in the middle and absent (index = width, index = r - 1), another one per assignment"""
    cycle = [0, width - 1, width // 2, width, r - 1]
    return [cycle[(i + shift) % len(cycle)] for i in range(count)]


def _decoder_key(gpu_ctx, curve, width):
    from polymath_amd import circuits as PC
    return _cached((curve, "decoder", width), lambda: _setup(gpu_ctx, curve, PC.Decoder(width, 0), 14000 + width))


# ---- 1. Decoder: one level of W indicator rows, at the chain / level threshold and the wave and workgroup edges of k_solve_indicator ------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("width", [1, 31, 32, 64, 257])
def test_decoder(gpu_ctx, curve, width):
    from polymath_amd import circuits as PC, polymath as PM
    r = CURVES[curve].r
    s = _decoder_key(gpu_ctx, curve, width)
    q = s["q"]
    assert (q.m0, q.mw, q.nr) == (2, 1 + width, width + 2)
    partial = PC.Decoder(width, 0).partial(r)
    assert partial == ([1, None], [0] + [PM.INDICATOR] * width)
    for count, shift in ((1, 2), (3, 0), (3, 3), (70, 1)):
        indices = _indices(width, r, count, shift)
        assignments = [PC.Decoder(width, index).native(r) for index in indices]
        for index, (inst, wit) in zip(indices, assignments):
            assert inst == [1, int(index < width)] and sum(wit[1:]) == inst[1] and (index >= width or wit[1 + index] == 1)
        _completes(s, assignments, partial)


# ---- 2. the shape variants, by hand; and two guards with the same constant ---------------------------------------------------------------------------
# columns: 0 one | 1 success (public) | 2 inp, 3 a, 4 b (given) | 5 u0, 6 u1, 7 u2, 8 u3 (indicators)
#   row 0: (3 - inp) * 7 u0 = 0      u in B, k = 7, the guard i - inp
#   row 1: u1 * (a - b) = 0          a guard between two signals
#   row 2: u2 * (inp - 3) = 0        the same constant as row 0
#   row 3: u3 * (inp - 5) = 0
#   row 4: (u0 + u1 + u2 + u3) * 1 = success      row 5: success * (success - 1) = 0
def variants_system(r):
    from polymath_amd.polymath import R1CS
    a = [[(3, 0), (r - 1, 2)], [(1, 6)], [(1, 7)], [(1, 8)], [(1, 5), (1, 6), (1, 7), (1, 8)], [(1, 1)]]
    b = [[(7, 5)], [(1, 3), (r - 1, 4)], [(1, 2), (r - 3, 0)], [(1, 2), (r - 5, 0)], [(1, 0)], [(1, 1), (r - 1, 0)]]
    c = [[], [], [], [], [(1, 1)], []]
    return R1CS(2, 7, a, b, c)


def _variants_assignment(inp, a, b):
    u = [int(inp == 3), int(a == b), int(inp == 3), int(inp == 5)]
    return [1, sum(u)], [inp, a, b] + u


@pytest.mark.parametrize("curve", BOTH)
def test_shape_variants(gpu_ctx, curve):
    from polymath_amd import polymath as PM
    r = CURVES[curve].r
    s = _cached((curve, "variants"), lambda: _setup(gpu_ctx, curve, (variants_system(r),) + tuple(_variants_assignment(5, 1, 2)), 14100))
    partial = ([1, None], [0, 0, 0] + [PM.INDICATOR] * 4)
    inputs = [(5, 1, 2), (4, 7, 7), (9, 1, 2), (3, 1, 2), (r - 1, r - 1, r - 1), (3, 0, r - 1)]
    assignments = [_variants_assignment(*v) for v in inputs]
    assert [inst[1] for inst, _ in assignments] == [1, 1, 0, 2, 1, 2]
    want, rows = _rows(s, assignments, partial)
    n_bad, bad_rows, stuck, full = _solve(s, rows)
    # inp = 3: both guards with the constant 3 store 1, success = 2 and the booleanity row 5 fails -- a failing row like any other
    assert stuck == [NONE] * 6 and n_bad == [0, 0, 0, 1, 0, 1], (stuck, n_bad)
    assert [int(bad_rows[i][0]) for i in (3, 5)] == [5, 5]
    assert np.array_equal(full, want)


# ---- 3. TableWalk: indicator levels and ordinary ones in turn; one chain launch, or wide launches; in order, reversed and shuffled ------------------
def _walk_inputs(g, width, steps, count, table=None):
    """per assignment (table, start): entries in range -- but every third assignment leads out of the table: through one entry, or
    (where the table is the circuit's own) from the start"""
    out = []
    for i in range(count):
        t = list(table) if table is not None else [g.next_u64() % width for _ in range(width)]
        start = g.next_u64() % width
        if i % 3 == 2 and table is None:
            t[g.next_u64() % width] = width + 3
        elif i % 3 == 2:
            start = width + 3
        out.append((t, start))
    return out


WALKS = [(8, 40, False), (8, 40, True), (40, 6, True)]


def _walk_key(gpu_ctx, curve, width, steps, signals, order):
    from polymath_amd import circuits as PC
    table = [(5 * i + 3) % width for i in range(width)]
    wrap = (lambda c: c) if order is None else (lambda c: PC.Reordered(c, order))
    s = _cached((curve, "walk", width, steps, signals, order), lambda: _setup(gpu_ctx, curve, wrap(PC.TableWalk(table, 1, steps, signals)), 14200 + width))
    return s, table


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("width,steps,signals", WALKS)
@pytest.mark.parametrize("order", [None, "reverse", 9103])
def test_table_walk(gpu_ctx, curve, width, steps, signals, order):
    from polymath_amd import circuits as PC, polymath as PM
    r = CURVES[curve].r
    s, table = _walk_key(gpu_ctx, curve, width, steps, signals, order)
    q = s["q"]
    per = 2 * width + 2 if signals else width + 2
    assert (q.m0, q.mw, q.nr) == (2, 1 + (width if signals else 0) + steps * per - 1, steps * (per + 1))
    partial = PC.TableWalk(table, 1, steps, signals).partial(r)
    assert sum(v is PM.INDICATOR for v in partial[1]) == steps * width and sum(v is not None and v is not PM.INDICATOR for v in partial[1]) == 1 + (width if signals else 0)
    g = PC.SplitMix64(14300 + width)
    for count in ((1, 70) if order is None else (3,)):
        inputs = _walk_inputs(g, width, steps, count, None if signals else table)
        assignments = [PC.TableWalk(t, start, steps, signals).native(r) for t, start in inputs]
        for (t, start), (inst, _) in zip(inputs, assignments):
            assert inst == [1, PC.table_walk_native(t, start, steps, r)]
        full = _completes(s, assignments, partial)
        if order is not None:      # the same words as the circuit in its own row order gives
            plain, _ = _walk_key(gpu_ctx, curve, width, steps, signals, None)
            assert np.array_equal(_completes(plain, assignments, partial), full)


# ---- 4. inputs -> verified proofs: the same bytes as the same call on the host-synthesised assignment ----------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_inputs_to_proofs(gpu_ctx, curve):
    from polymath_amd import circuits as PC
    r, count, width, steps = CURVES[curve].r, 5, 8, 40
    s, _ = _walk_key(gpu_ctx, curve, width, steps, True, None)
    pm, pk, f, q = s["pm"], s["pk"], s["f"], s["q"]
    g = PC.SplitMix64(14400)
    circuits = [PC.TableWalk(t, start, steps) for t, start in _walk_inputs(g, width, steps, count)]
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
    proofs = None
    for glue in ("host", "device"):
        proofs, statuses, instances = pm.prove_batch(pk, part, r_as, solve=True, glue=glue)
        plain_proofs, plain_statuses = pm.prove_batch(pk, full, r_as, glue=glue)
        assert statuses == [0] * count and plain_statuses == [0] * count and instances == [inst for inst, _ in assignments], glue
        assert proofs == plain_proofs and proofs[1] == solved, glue
        assert all(pm.verify(vk, assignments[i][0][1:], proofs[i]) for i in range(count)), glue
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


# ---- 5. an indicator column that is a public input: the hashed instance carries the solved value under both glue modes ----------------------------
# columns: 0 one | 1 out (public, the indicator) | 2 inp, 3 w (given).   row 0: out * (inp - 2) = 0      row 1: inp * w = inp w (a check row)
def public_system(r):
    from polymath_amd.polymath import R1CS
    return R1CS(2, 3, [[(1, 1)], [(1, 2)]], [[(1, 2), (r - 2, 0)], [(1, 3)]], [[], [(1, 4)]])


@pytest.mark.parametrize("curve", BOTH)
def test_indicator_as_public_input(gpu_ctx, curve):
    from polymath_amd import polymath as PM
    r = CURVES[curve].r
    s = _cached((curve, "public"), lambda: _setup(gpu_ctx, curve, (public_system(r), [1, 1], [2, 5, 10]), 14500))
    pm, pk, f, q = s["pm"], s["pk"], s["f"], s["q"]
    inputs = [2, 7, 2, 0, r - 1]
    count = len(inputs)
    assignments = [([1, int(inp == 2)], [inp, 5, 5 * inp % r]) for inp in inputs]
    want, rows = _rows(s, assignments, ([1, PM.INDICATOR], [0, 0, 0]))
    from polymath_amd import api
    assert tuple(int(v) for v in rows[0, 1]) == api.INDICATOR_LIMBS
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
        assert not pm.verify(vk, [1 - assignments[0][0][1]], proofs[0]), glue                        # the value that was hashed is the solved one
    rc, one = pk.host_prove("merlin", part[1][0], part[1][0], part[1][1], f.fr_limbs(r_as[1]), solve=True)
    assert rc == PM_OK and one == proofs[1]


# ---- 6. the marker is explicit: the plain marker is stuck at the hit row, mixed markers are a mismatch ----------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("width", [31, 32])
def test_plain_marker_is_stuck_at_the_hit(gpu_ctx, curve, width):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    s = _decoder_key(gpu_ctx, curve, width)
    indices = [0, width, width - 1, width // 2, r - 1]
    assignments = [PC.Decoder(width, index).native(r) for index in indices]
    partial = PC.Decoder(width, 0).partial(r)
    plain = (partial[0], [None if j else v for j, v in enumerate(partial[1])])
    want, rows = _rows(s, assignments, plain)
    n_bad, bad_rows, stuck, full = _solve(s, rows)
    # guard row i is row i: an index in range divides by zero there, an index out of range completes
    assert stuck == [0, NONE, width - 1, width // 2, NONE] and n_bad == [NONE, 0, NONE, NONE, 0]
    assert int(bad_rows[2][0]) == width - 1 and np.array_equal(full[1], want[1]) and np.array_equal(full[4], want[4])
    # the same rows with the indicator marker: every assignment completes, so the marker is what makes the difference
    _completes(s, assignments, partial)


@pytest.mark.parametrize("curve", BOTH)
def test_mixed_markers_are_a_mismatch(gpu_ctx, curve):
    from polymath_amd import circuits as PC
    r, width = CURVES[curve].r, 31
    s = _decoder_key(gpu_ctx, curve, width)
    pm, pk, q = s["pm"], s["pk"], s["q"]
    assignments = [PC.Decoder(width, index).native(r) for index in (3, 30, 31)]
    partial = PC.Decoder(width, 0).partial(r)
    want, rows = _rows(s, assignments, partial)
    column = q.m0 + 1 + 12
    mixed = rows.copy()
    mixed[1, column] = (NONE,) * 4                                          # assignment 1 marks out_12 with the plain marker
    rc, n_bad, bad_rows, _ = pk.r1cs_check_batch(np.ascontiguousarray(mixed[:, :q.m0]), np.ascontiguousarray(mixed[:, q.m0:]), 2, solve=True)
    assert rc == PM_ERR_INVALID_ARG and "assignment 1 differs from assignment 0 at column %d" % column in pm.ctx.last_error(), pm.ctx.last_error()
    part = [(np.ascontiguousarray(mixed[i, :q.m0]), np.ascontiguousarray(mixed[i, q.m0:])) for i in range(3)]
    with pytest.raises(Exception):
        pm.prove_batch(pk, part, [[3, 5]] * 3, solve=True)
    assert "assignment 1 differs from assignment 0 at column %d" % column in pm.ctx.last_error()
    # the refused batch left nothing behind: the context is as usable as before
    _completes(s, assignments, partial)
