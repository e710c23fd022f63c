"""k_accumulate's schedule (msm.hip): a grid of resident workgroups whose waves draw 64 task descriptors at a time from a
per-context ticket counter.  Bit-exact against the CPU restatement where that schedule differs most from one lane per task:
fewer tasks than resident lanes, many rounds of multi-task buckets, no tasks at all, hot-bucket tiers, the wide mode, and two
contexts drawing tickets at the same time."""
import threading

import numpy as np
import pytest

from helpers import TABLES_OPT, rand_fr_limbs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from polymath_amd import api as _api
    return _api


def _both_paths(bases, sc, ref, rinf):
    """The per-window pipeline (plain bases), then the table pipeline (window tables) on the same scalars."""
    out, inf = bases.msm(sc)
    assert inf == rinf and (np.array_equal(out, ref) if ref is not None else not out.any())
    bases.precompute()
    out, inf = bases.msm(sc)
    assert inf == rinf and (np.array_equal(out, ref) if ref is not None else not out.any())


@pytest.mark.parametrize("n", [1, 40, 5000])
def test_fewer_tasks_than_resident_lanes(gpu_ctx, oracle, api, n):
    curve = "bls12_381"
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    sc = rand_fr_limbs(curve, n, 4100 + n)
    ref, rinf = oracle.msm(curve, bases.download(), sc, 8)
    _both_paths(bases, sc, ref, rinf)


@pytest.mark.parametrize("curve,log_n,task_len", [("bls12_381", 18, 64), ("bn254", 17, 0)])
def test_many_rounds_and_multi_task_buckets(gpu_ctx, oracle, api, curve, log_n, task_len):
    """2^18 pairs in 64-entry tasks: every bucket owns several tasks and the waves draw many tickets each; BN254 at the
    automatic task length."""
    if task_len:
        gpu_ctx.set_option("msm_task_len", task_len)
    n = 1 << log_n
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    sc = rand_fr_limbs(curve, n, 4200 + log_n)
    ref, rinf = oracle.msm(curve, bases.download(), sc, 8)
    _both_paths(bases, sc, ref, rinf)


def test_zero_tasks(gpu_ctx, api):
    """All-zero scalars: no bucket has an entry, the ticket's first draw already ends every wave."""
    curve, n = "bls12_381", 4096
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    _both_paths(bases, np.zeros((n, 4), dtype=np.uint64), None, 1)


def test_hot_bucket_tiers(gpu_ctx, oracle, api):
    """One scalar repeated over most pairs (a bucket per window with more than 1024 tasks: the workgroup fold), a second over a
    few hundred (the wave fold), random ones between: the long descriptors of a hot bucket sit in front of the rest."""
    curve, n = "bls12_381", 1 << 16
    gpu_ctx.set_option("msm_task_len", 64)
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    vals = rand_fr_limbs(curve, 2, 4301)
    sc = np.repeat(vals[:1], n, axis=0)
    sc[1::101] = vals[1]
    sc[::7] = rand_fr_limbs(curve, len(sc[::7]), 4302)
    ref, rinf = oracle.msm(curve, bases.download(), sc, 8)
    _both_paths(bases, sc, ref, rinf)


def test_wide_mode_matches_tables(gpu_ctx):
    """A whole proof whose MSMs run in the wide mode (one bucket set per window, plain bases gathered by the same kernel)
    gives the bytes of the proof with window tables, at the automatic and at a short task length."""
    from polymath_amd import circuits as PC
    from polymath_amd.polymath import Polymath
    curve = "bls12_381"
    lc = PC.synthetic_r1cs_native(curve, 5000)
    pm = Polymath(curve, "keccak256", ctx=gpu_ctx)
    proofs = []
    for tables in ("1", "wide"):
        gpu_ctx.set_option("tables", TABLES_OPT[tables])
        pk = pm.setup(lc, 0x5EED, 0xC0FFEE)
        assert pk.msm_plan(2)[3] == (tables == "1")
        for task_len in (0, 64):
            gpu_ctx.set_option("msm_task_len", task_len)
            proofs.append(pm.prove_native(pk, lc.inst_limbs, lc.wit_limbs, [3, 11]))
        pk.free()
    assert all(p == proofs[0] for p in proofs)


def test_two_contexts_draw_tickets_at_once(oracle, api):
    """Two host threads, each with its own context (and so its own ticket counter), run table-mode MSMs over the same bases at
    the same time, several rounds each: every result equals the CPU restatement's."""
    curve, n, ROUNDS = "bls12_381", 1 << 16, 4
    ctxs = [api.Context(0) for _ in range(2)]
    try:
        bases = [api.Bases.multiples(c, curve, n) for c in ctxs]
        for b in bases:
            b.precompute()
        hb = bases[0].download()
        assert np.array_equal(bases[1].download(), hb)
        scs = [rand_fr_limbs(curve, n, 4400 + i) for i in range(2)]
        want = [oracle.msm(curve, hb, s, 8) for s in scs]
        got, errs = [[None] * ROUNDS for _ in range(2)], [None] * 2
        start = threading.Barrier(2)

        def body(i):
            try:
                start.wait(60)
                for k in range(ROUNDS):
                    got[i][k] = bases[i].msm(scs[(i + k) % 2])
            except BaseException as e:     # noqa: BLE001
                errs[i] = e
        th = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(300)
        assert not any(t.is_alive() for t in th)
        assert errs == [None] * 2, errs
        for i in range(2):
            for k in range(ROUNDS):
                out, inf = got[i][k]
                ref, rinf = want[(i + k) % 2]
                assert inf == rinf and np.array_equal(out, ref), (i, k)
        for b in bases:
            b.free()
    finally:
        for c in ctxs:
            c.close()
