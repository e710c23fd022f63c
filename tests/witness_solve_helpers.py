"""What the GPU tests of PM_ASSIGNMENT_SOLVE (tests/test_gpu_witness_solve*.py) share: a key per (curve, circuit), partial assignments as
limb rows with the three markers, the solve call and the check that a batch completes.  A plain module, imported by name; a helper
that differs in one test file stays in that file."""
import numpy as np

from oracle.pyref.fields import CURVES

PM_OK, PM_ERR_INVALID_ARG = 0, 1
NONE = (1 << 64) - 1
BOTH = ["bls12_381", "bn254"]


def _setup(gpu_ctx, curve, circuit, seed):
    """circuit: a generator of polymath_amd.circuits, or an (R1CS, instance, witness) triple"""
    from polymath_amd import circuits as PC, polymath as PM
    c = CURVES[curve]
    g = PC.SplitMix64(seed)
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    x, z = g.fr(c.r), g.fr(c.r)
    q, inst, wit = pm._synthesize(circuit)
    pk = pm.setup((q, inst, wit), x, z)
    return dict(pm=pm, pk=pk, q=q, inst=inst, wit=wit, x=x, z=z, f=pm.field, c=c)


def key_cache():
    """-> _cached(key, make) over a dictionary of its own: one per test module, so that two modules may use the same key"""
    keys = {}

    def _cached(key, make):
        if key not in keys:
            keys[key] = make()
        return keys[key]
    return _cached


def _limbs(s, values):
    """fr_limbs(values).reshape(-1, 4); the many zeros and ones (bits, indicators) come from a table"""
    f = s["f"]
    small = np.fromiter((v if v <= 1 else 0 for v in values), dtype=np.intp, count=len(values))
    out = f.fr_limbs([0, 1]).reshape(2, 4)[small]
    big = np.fromiter((v > 1 for v in values), dtype=bool, count=len(values))
    if big.any():
        out[big] = f.fr_limbs([v for v in values if v > 1]).reshape(-1, 4)
    return out


def _full_limbs(s, inst, wit):
    return np.concatenate([s["f"].fr_limbs(inst), s["f"].fr_limbs(wit)]).reshape(-1, 4)


def _rows(s, assignments, partial):
    """assignments: [(instance, witness)] as ints; partial: (instance, witness) with None, PM.QUOTIENT or PM.INDICATOR where the device solves
    -> (want, rows): count x (m0 + mw) x 4 words; want = the full assignments, rows = the same with the partial's markers"""
    from polymath_amd import api, polymath as PM
    want = np.stack([_limbs(s, list(inst) + list(wit)) for inst, wit in assignments])
    marks = list(partial[0]) + list(partial[1])
    rows = want.copy()
    for mark, limbs in ((None, api.UNKNOWN_LIMBS), (PM.QUOTIENT, api.QUOTIENT_LIMBS), (PM.INDICATOR, api.INDICATOR_LIMBS)):
        rows[:, np.array([v is mark for v in marks], dtype=bool)] = limbs
    return want, rows


def _solve(s, rows, max_rows=2):
    """r1cs_check_batch(solve=True) on host limb rows -> (n_bad, bad rows, stuck words, completed x || w rows)"""
    m0 = s["q"].m0
    xs, ws = np.ascontiguousarray(rows[:, :m0]), np.ascontiguousarray(rows[:, m0:])
    rc, n_bad, bad_rows, _ = s["pk"].r1cs_check_batch(xs, ws, max_rows, solve=True)
    assert rc == PM_OK, s["pm"].ctx.last_error()
    stuck, _ = s["pk"].solve_results(len(xs))
    return [int(v) for v in n_bad], bad_rows, [int(v) for v in stuck], s["pk"].solved_assignments(len(xs), s["q"].mw)


def _completes(s, assignments, partial):
    want, rows = _rows(s, assignments, partial)
    n_bad, _, stuck, full = _solve(s, rows)
    count = len(assignments)
    assert n_bad == [0] * count and stuck == [NONE] * count, (count, n_bad, stuck)
    assert np.array_equal(full, want), count
    return full
