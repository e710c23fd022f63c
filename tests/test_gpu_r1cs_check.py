"""GPU: pm_r1cs_check / pm_r1cs_check_batch (Polymath.check_assignment / check_batch) -- which R1CS rows an assignment violates.
The bar is equality with Python integers: per row r, (Az)_r, (Bz)_r, (Cz)_r come from oracle.pyref.circuits.first_entry_dot (the
first-entry rule of common.rs:100-105); n_bad, the ascending list with its UINT64_MAX padding and the residuals must be those, and
n_bad > 0 must hold exactly where the prover returns PM_ERR_REMAINDER_NONZERO.

Shapes are the smallest at which each mechanism can differ.  The mask kernel runs 256-lane workgroups of four waves: nr = 500 is two
workgroups with a partial last wave, nr = 1 and nr = 64 are one partial / one whole wave.  The scan walks SCAN_ROWS = 2^14 rows (256 mask
words) per iteration: nr = SCAN_ROWS + 200 crosses one carry (n = 2^16)."""
import ctypes as ct

import numpy as np
import pytest

from oracle.pyref import circuits as CI
from oracle.pyref.fields import CURVES

pytestmark = pytest.mark.gpu

PM_OK, PM_ERR_INVALID_ARG, PM_ERR_REMAINDER_NONZERO = 0, 1, 4
NO_ROW = (1 << 64) - 1
SCAN_ROWS = 1 << 14            # r1cs_check.hip: R1CS_SCAN_ROWS, the scan's per-iteration coverage
_KEYS = {}


# ---- ground truth on Python integers ----------------------------------------------------------------------------------------------
def expected(c, q, inst, wit, max_rows):
    """(n_bad, rows padded to max_rows, [(az, bz, cz)] of the listed rows)"""
    zz = list(inst) + list(wit)
    bad, abc = [], []
    for r, (ra, rb, rc) in enumerate(zip(q.a, q.b, q.c)):
        az, bz, cz = CI.first_entry_dot(c.r, ra, zz), CI.first_entry_dot(c.r, rb, zz), CI.first_entry_dot(c.r, rc, zz)
        if az * bz % c.r != cz:
            bad.append(r)
            if len(abc) < max_rows:
                abc.append((az, bz, cz))
    listed = bad[:max_rows]
    return len(bad), listed + [NO_ROW] * (max_rows - len(listed)), abc


def assert_check(pm, pk, c, q, inst, wit, max_rows):
    """pm_r1cs_check with residuals on host limbs == Python; -> n_bad"""
    f = pm.field
    want_n, want_rows, want_abc = expected(c, q, inst, wit, max_rows)
    rc, n_bad, rows, abc = pk.r1cs_check(f.fr_limbs(inst), f.fr_limbs(wit), max_rows, residuals=True)
    assert rc == PM_OK
    assert n_bad == want_n
    assert [int(v) for v in rows] == want_rows
    got_abc = [tuple(f.fr_int(abc[j, k]) for k in range(3)) for j in range(len(want_abc))]
    assert got_abc == want_abc
    assert not abc[len(want_abc):].any()                       # unused slots are zero
    return n_bad


# ---- the diagonal circuit: row r is  w[r] * 1 = w[nr + r], so changing w[nr + r] makes row r fail and only row r --------------------
def diagonal(c, nr, seed=1):
    g = CI.SplitMix64(5000 + nr + seed)
    t = [g.fr(c.r) for _ in range(nr)]
    q = CI.R1CS(1, 2 * nr, [[(1, 1 + r)] for r in range(nr)], [[(1, 0)] for _ in range(nr)], [[(1, 1 + nr + r)] for r in range(nr)])
    return q, [1], t + t


def corrupt(c, wit, nr, rows):
    wit = list(wit)
    for r in rows:
        wit[nr + r] = (wit[nr + r] + 1 + r) % c.r
    return wit


def _setup(gpu_ctx, curve, q, inst, wit, seed):
    from polymath_amd import polymath as PM
    c = CURVES[curve]
    g = CI.SplitMix64(seed)
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    pk = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), inst, wit), g.fr(c.r), g.fr(c.r))
    return pm, pk


def _diag_key(gpu_ctx, curve, nr):
    if (curve, nr) not in _KEYS:
        q, inst, wit = diagonal(CURVES[curve], nr)
        pm, pk = _setup(gpu_ctx, curve, q, inst, wit, 88 + nr)
        _KEYS[(curve, nr)] = dict(pm=pm, pk=pk, q=q, inst=inst, wit=wit)
    return _KEYS[(curve, nr)]


def _status(pm, pk, inst, wit, r_a=(3, 5)):
    from polymath_amd.polymath import PolymathProverError
    try:
        return 0, pm.prove_native(pk, pm.field.fr_limbs(inst), pm.field.fr_limbs(wit), list(r_a))
    except PolymathProverError as e:
        return e.status, None


# ---- 1. wave and block edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_wave_and_block_edges(gpu_ctx, curve):
    c = CURVES[curve]
    s = _diag_key(gpu_ctx, curve, 500)
    for failing in ([], [0], [499], [63, 64], [255, 256], [0, 63, 64, 255, 256, 499]):
        wit = corrupt(c, s["wit"], 500, failing)
        assert assert_check(s["pm"], s["pk"], c, s["q"], s["inst"], wit, 8) == len(failing), failing
    wit = corrupt(c, s["wit"], 500, range(500))
    assert assert_check(s["pm"], s["pk"], c, s["q"], s["inst"], wit, 503) == 500      # every row listed, three slots of padding
    assert assert_check(s["pm"], s["pk"], c, s["q"], s["inst"], wit, 8) == 500


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
@pytest.mark.parametrize("nr", [1, 64])
def test_one_wave(gpu_ctx, curve, nr):
    c = CURVES[curve]
    s = _diag_key(gpu_ctx, curve, nr)
    for failing in ([], [0], [nr - 1], list(range(nr))):
        wit = corrupt(c, s["wit"], nr, failing)
        assert assert_check(s["pm"], s["pk"], c, s["q"], s["inst"], wit, 8) == len(set(failing)), failing


# ---- 2. truncation ------------------------------------------------------------------------------------------------------------------------
def test_truncation(gpu_ctx):
    curve = "bls12_381"
    c = CURVES[curve]
    s = _diag_key(gpu_ctx, curve, 500)
    pm, pk, f = s["pm"], s["pk"], s["pm"].field
    failing = [0, 63, 64, 255, 256, 499]
    wit = corrupt(c, s["wit"], 500, failing)
    assert assert_check(pm, pk, c, s["q"], s["inst"], wit, 4) == 6
    xl, wl = f.fr_limbs(s["inst"]), f.fr_limbs(wit)
    rc, n_bad, rows, abc = pk.r1cs_check(xl, wl, 4)                      # abc = NULL
    assert (rc, n_bad, [int(v) for v in rows], abc) == (PM_OK, 6, failing[:4], None)
    rc, n_bad, rows, abc = pk.r1cs_check(xl, wl, 0)                      # max_rows = 0, rows = NULL: the count only
    assert (rc, n_bad, len(rows), abc) == (PM_OK, 6, 0, None)
    rc, n_bad, rows, abc = pk.r1cs_check(xl, wl, 0, residuals=True)
    assert (rc, n_bad) == (PM_OK, 6)
    assert pm.check_assignment(pk, (xl, wl), max_rows=4, residuals=True) == (6, failing[:4], expected(c, s["q"], s["inst"], wit, 4)[2])
    assert pm.check_assignment(pk, (xl, wl)) == (6, failing)
    t = gpu_ctx.timings()
    assert t["witness_map"] > 0 and all(v == 0 for k, v in t.items() if k != "witness_map"), t


# ---- 3. the scan's carry ---------------------------------------------------------------------------------------------------------------
def test_scan_carry(gpu_ctx):
    curve = "bls12_381"
    c = CURVES[curve]
    nr = SCAN_ROWS + 200
    s = _diag_key(gpu_ctx, curve, nr)
    assert s["pk"].n == 1 << 16
    failing = [SCAN_ROWS - 1, SCAN_ROWS, nr - 1]
    wit = corrupt(c, s["wit"], nr, failing)
    want = [(s["wit"][r], 1, wit[nr + r]) for r in failing]
    f = s["pm"].field
    rc, n_bad, rows, abc = s["pk"].r1cs_check(f.fr_limbs(s["inst"]), f.fr_limbs(wit), 8, residuals=True)
    assert (rc, n_bad, [int(v) for v in rows]) == (PM_OK, 3, failing + [NO_ROW] * 5)
    assert [tuple(f.fr_int(abc[j, k]) for k in range(3)) for j in range(3)] == want and not abc[3:].any()
    rc, n_bad, rows, _ = s["pk"].r1cs_check(f.fr_limbs(s["inst"]), f.fr_limbs(wit), 2)       # the list ends inside the first iteration
    assert (rc, n_bad, [int(v) for v in rows]) == (PM_OK, 3, failing[:2])
    rc, n_bad, rows, _ = s["pk"].r1cs_check(f.fr_limbs(s["inst"]), f.fr_limbs(s["wit"]), 8)
    assert (rc, n_bad, [int(v) for v in rows]) == (PM_OK, 0, [NO_ROW] * 8)
    s["pk"].free()
    del _KEYS[(curve, nr)]


# ---- 4. first-entry semantics and the prover's verdict -------------------------------------------------------------------------------------
def _random_shape(seed):
    curve = ("bls12_381", "bn254")[seed % 2]
    m0 = 1 + seed                                                  # 1 .. 20
    nr = 9 + (seed * 7) % 40
    return curve, CI.random_r1cs(CURVES[curve], 0xC4EC + seed, m0, nr)


def _shape_features(q):
    """what the seeded shapes must cover between them"""
    rows = [row for m in (q.a, q.b, q.c) for row in m]
    used = {j for row in rows for _, j in row}
    return dict(duplicate=any(len({j for _, j in row}) < len(row) for row in rows), zero=any(v == 0 for row in rows for v, _ in row),
                empty=any(not row for row in rows), unused=any(j not in used for j in range(q.m0, q.m0 + q.mw)))


def test_random_shapes_cover_the_cases():
    seen = {}
    for seed in range(20):
        curve, (q, inst, wit) = _random_shape(seed)
        assert q.m0 == 1 + seed
        for k, v in _shape_features(q).items():
            seen[k] = seen.get(k, 0) + int(v)
    assert all(seen[k] >= 3 for k in ("duplicate", "zero", "empty", "unused")), seen


@pytest.mark.parametrize("seed", range(20))
def test_random_shapes_and_the_provers_verdict(gpu_ctx, seed):
    curve, (q, inst, wit) = _random_shape(seed)
    c = CURVES[curve]
    pm, pk = _setup(gpu_ctx, curve, q, inst, wit, 700 + seed)
    assert assert_check(pm, pk, c, q, inst, wit, 8) == 0
    assert _status(pm, pk, inst, wit)[0] == 0
    rows = [row for m in (q.a, q.b, q.c) for row in m]
    used = sorted({j for row in rows for _, j in row if j >= q.m0})
    unused = [j for j in range(q.m0, q.m0 + q.mw) if j not in used]
    some_fail = False
    for col in [used[seed % len(used)], used[(3 * seed + 1) % len(used)]] + unused[:1]:
        bad = list(wit)
        bad[col - q.m0] = (bad[col - q.m0] + 1 + seed) % c.r
        n_bad = assert_check(pm, pk, c, q, inst, bad, 8)
        status, proof = _status(pm, pk, inst, bad)
        assert (n_bad > 0) == (status == PM_ERR_REMAINDER_NONZERO) and status in (0, PM_ERR_REMAINDER_NONZERO), (col, n_bad, status)
        if col in unused:
            assert n_bad == 0 and proof is not None
        some_fail |= n_bad > 0
    assert some_fail
    pk.free()


@pytest.mark.parametrize("curve,rounds,n", [("bls12_381", 16, 1 << 7), ("bn254", 16, 1 << 7), ("bls12_381", 322, 1 << 11)])
def test_mimc(gpu_ctx, curve, rounds, n):
    c = CURVES[curve]
    g = CI.SplitMix64(4000 + rounds)
    q, inst, wit = CI.mimc_circuit(c, g.fr(c.r), g.fr(c.r), [g.fr(c.r) for _ in range(rounds)])
    pm, pk = _setup(gpu_ctx, curve, q, inst, wit, 900 + rounds)
    assert pk.n == n
    assert assert_check(pm, pk, c, q, inst, wit, 8) == 0 and _status(pm, pk, inst, wit)[0] == 0
    bad = list(wit)
    bad[len(bad) // 2] = (bad[len(bad) // 2] + 1) % c.r
    assert assert_check(pm, pk, c, q, inst, bad, 8) > 0 and _status(pm, pk, inst, bad)[0] == PM_ERR_REMAINDER_NONZERO
    pk.free()


# ---- 5. batch -------------------------------------------------------------------------------------------------------------------------------
def test_batch(gpu_ctx):
    import torch
    curve = "bls12_381"
    c = CURVES[curve]
    nr, count = 100, 5
    s = _diag_key(gpu_ctx, curve, nr)
    pm, pk, f, q = s["pm"], s["pk"], s["pm"].field, s["q"]
    assert q.m0 + q.mw == 201
    failing = {1: [7], 3: [0, 64, 99]}
    wits = []
    for i in range(count):
        g = CI.SplitMix64(6000 + i)
        t = [g.fr(c.r) for _ in range(nr)]
        wits.append(corrupt(c, t + t, nr, failing.get(i, [])))
    xs = np.stack([f.fr_limbs(s["inst"])] * count)
    ws = np.stack([f.fr_limbs(w) for w in wits])
    single = [pk.r1cs_check(xs[i], ws[i], 4, residuals=True) for i in range(count)]
    for i in range(count):
        assert single[i][0] == PM_OK and single[i][1] == len(failing.get(i, []))
        assert [int(v) for v in single[i][2]] == expected(c, q, s["inst"], wits[i], 4)[1]
    dx, dw = torch.from_numpy(xs.view(np.int64)).cuda(), torch.from_numpy(ws.view(np.int64)).cuda()
    torch.cuda.synchronize()

    def both():
        host = pk.r1cs_check_batch(xs, ws, 4, residuals=True)
        dev = pk.r1cs_check_batch(dx.data_ptr(), dw.data_ptr(), 4, residuals=True, on_device=True, count=count)
        for rc, n_bad, rows, abc in (host, dev):
            assert rc == PM_OK
            for i in range(count):
                assert int(n_bad[i]) == single[i][1]
                assert np.array_equal(rows[i], single[i][2]) and np.array_equal(abc[i], single[i][3]), i

    both()                                                    # one group
    assert 2 * 201 <= 1 << 9 < 3 * 201
    gpu_ctx.set_option("msm_max_piece_log", 9)                # groups of 2, 2, 1 (restored by conftest)
    both()
    got = pm.check_batch(pk, [(xs[i], ws[i]) for i in range(count)], max_rows=4)
    assert got == [(len(failing.get(i, [])), failing.get(i, [])) for i in range(count)]
    assert pm.check_batch(pk, count, max_rows=4, device_ptrs=(dx.data_ptr(), dw.data_ptr())) == got
    gpu_ctx.set_option("msm_max_piece_log", 27)
    # the batch prover refuses exactly the rows with n_bad > 0
    ra = np.stack([f.fr_limbs([11 + i, 13 + i]) for i in range(count)])
    rc, _, status = pk.host_prove_batch("merlin", xs, xs, ws, ra)
    assert rc == PM_OK and [int(v) for v in status] == [PM_ERR_REMAINDER_NONZERO if i in failing else 0 for i in range(count)]
    # count == 0 writes nothing
    n_bad, rows, abc = np.full(2, 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint64), np.full(96, 77, dtype=np.uint64)
    from polymath_amd import api
    vp = lambda a: a.ctypes.data_as(ct.c_void_p)
    assert gpu_ctx.L.pm_r1cs_check_batch(gpu_ctx.h, pk.h, 0, vp(xs), vp(ws), 0, 4, api._p(n_bad), api._p(rows), api._p(abc)) == PM_OK
    assert gpu_ctx.L.pm_r1cs_check_batch(gpu_ctx.h, pk.h, 0, None, None, 0, 4, None, None, None) == PM_OK
    assert (n_bad == 77).all() and (rows == 77).all() and (abc == 77).all()
    assert pm.check_batch(pk, []) == []


# ---- 6. a proof in flight is not disturbed ----------------------------------------------------------------------------------------------
def test_proof_in_flight_is_not_disturbed(gpu_ctx):
    curve = "bls12_381"
    c = CURVES[curve]
    s = _diag_key(gpu_ctx, curve, 100)
    pm, pk, f = s["pm"], s["pk"], s["pm"].field
    xl, wl = f.fr_limbs(s["inst"]), f.fr_limbs(s["wit"])
    bad = f.fr_limbs(corrupt(c, s["wit"], 100, [5, 70]))
    r_a = [21, 34]
    want = pm.prove_native(pk, xl, wl, r_a)
    seen = []
    phase2, phase3 = pk.phase2, pk.phase3

    def checked(phase):
        def run(*args):                                       # pm_r1cs_check between the phases of the proof in flight
            seen.append(pk.r1cs_check(xl, bad, 4, residuals=True)[:3])
            return phase(*args)
        return run
    pk.phase2, pk.phase3 = checked(phase2), checked(phase3)
    try:
        proof = pm.prove_limbs(pk, s["inst"], xl, wl, r_a)
    finally:
        del pk.phase2, pk.phase3
    assert len(seen) == 2 and all((rc, n, [int(v) for v in rows]) == (PM_OK, 2, [5, 70, NO_ROW, NO_ROW]) for rc, n, rows in seen)
    assert proof.to_bytes() == want
    assert pm.prove_native(pk, xl, wl, r_a) == want


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_alone(gpu_ctx):
    """Every PM_ERR_INVALID_ARG case of the contract.  The key on another device needs a second GPU and is checked where one is
    visible."""
    from polymath_amd import api, polymath as PM
    curve = "bls12_381"
    s = _diag_key(gpu_ctx, curve, 100)
    pm, pk, f, q = s["pm"], s["pk"], s["pm"].field, s["q"]
    xs, ws = np.stack([f.fr_limbs(s["inst"])] * 2), np.stack([f.fr_limbs(s["wit"])] * 2)
    n_bad, rows, abc = np.full(2, 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint64), np.full(96, 77, dtype=np.uint64)
    L, vp = gpu_ctx.L, lambda a: a.ctypes.data_as(ct.c_void_p)
    half = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), s["inst"], s["wit"]), 123, 456, 0, 2)        # PM_SHARD_PAIRS, shard_count = 2
    cases = [("sharded key", (gpu_ctx.h, half.h, 2, vp(xs), vp(ws), 0, 4, api._p(n_bad), api._p(rows), api._p(abc))),
             ("NULL n_bad", (gpu_ctx.h, pk.h, 2, vp(xs), vp(ws), 0, 4, None, api._p(rows), api._p(abc))),
             ("NULL rows", (gpu_ctx.h, pk.h, 2, vp(xs), vp(ws), 0, 4, api._p(n_bad), None, api._p(abc))),
             ("NULL x", (gpu_ctx.h, pk.h, 2, None, vp(ws), 0, 4, api._p(n_bad), api._p(rows), api._p(abc))),
             ("NULL w", (gpu_ctx.h, pk.h, 2, vp(xs), None, 0, 4, api._p(n_bad), api._p(rows), api._p(abc)))]
    other = None
    if L.pm_device_count() > 1:
        other = api.Context(1)
        cases.append(("key on another device", (other.h, pk.h, 2, vp(xs), vp(ws), 0, 4, api._p(n_bad), api._p(rows), api._p(abc))))
    for name, args in cases:
        assert L.pm_r1cs_check_batch(*args) == PM_ERR_INVALID_ARG, name
        assert L.pm_r1cs_check(*(args[:2] + args[3:])) == PM_ERR_INVALID_ARG, name
        assert (n_bad == 77).all() and (rows == 77).all() and (abc == 77).all(), name
    half.free()
    if other is not None:
        other.close()
    # the context is as usable as before
    assert pm.check_assignment(pk, (xs[0], ws[0])) == (0, [])
