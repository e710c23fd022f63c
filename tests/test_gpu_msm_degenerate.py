"""GPU: MSM inputs on which point additions DEGENERATE -- a + (-a) = O, a + a, O + a -- at every place the bucket pipelines add.

The kernels add with incomplete XYZZ formulas on reduced-radix registers and hand a = +-b to a cold path (fq28.cuh:
xyzz28_madd_exceptional for k_accumulate, xyzz28_add_exceptional for k_bucket_reduce / k_task_fold / k_sum_parts / the LDS trees
and, behind the four-lane xyzz28_add_quad, for k_reduce_level0 / level1 / final; dense xyzz_add / xyzz_dbl in host_horner, the sum
over pieces and pm_g1_sum).  The fast paths know the identity by ZZ being zero in every limb, so a cancellation that returns any
other representative of O, or takes the doubling branch, corrupts every later addition.  Generic inputs (distinct multiples
in index order, random scalars) never add opposite points anywhere; these do, on purpose, in every stage.

Every base is a known multiple k_i G (helpers.signed_multiples), so each MSM has two independent expectations, asserted equal to
each other (helpers.msm_two_references: the CPU restatement's Pippenger with complete additions, and the closed form
(sum s_i k_i mod r) G) and bit-equal to the GPU's affine limbs and infinity flag, `out` all zero with the flag.
test_msm_degenerate_inputs.py checks the same inputs and references on the CPU.  The families (helpers.family_a ... family_f,
FAMILY_G) each run on both curves and on four pipelines (helpers.msm_pipeline): per-window Pippenger at 2^17 pairs; window tables
of 16 bits at 2^17 (2^15 buckets: the two-level reduction); window tables with 2^11 buckets at 2^11 pairs (single-level reduction,
one sort region -- forced with table_window_bits = 12, the cost model's own choice at that size is a wider window); and the
cost model's tables at 2^17.

NOT covered: the wide plan (api.hip: PM_TABLES_WIDE) is reachable only through a proving key, whose MSM scalars come from the
prover; it shares accumulate<C, false> and reduce_two_level with the pipelines here, its own sort front end and the
multi-set launches of the reduction see no crafted cancellation."""
import numpy as np
import pytest

from helpers import (FAMILY_G, PIPELINE_NAMES, family_a, family_b, family_c, family_d, family_e, family_f, msm_pipeline, msm_two_references,
                     scalar_limbs, signed_multiples)
from oracle.pyref.fields import CURVES

pytestmark = pytest.mark.gpu

CURVE_LIST = ["bls12_381", "bn254"]
E_VECTORS = 12          # seeded scalar vectors of family E per pipeline


@pytest.fixture(scope="module")
def api():
    from polymath_amd import api as _api
    return _api


def _resident(api, ctx, curve, pipe, hb):
    """hb on the GPU under the pipeline's options (restored after the test by conftest), with window tables where it has them"""
    for k, v in pipe["options"].items():
        ctx.set_option(k, v)
    bases = api.Bases.upload(ctx, curve, hb)
    if pipe["tables"]:
        bases.precompute()
    return bases


def _check(bases, curve, want, winf, scalars, label, offset=0):
    n = len(scalars) if not isinstance(scalars, dict) else len(bases)
    out, inf = bases.msm(scalar_limbs(curve, n, scalars), offset=offset)
    ok = inf == winf and np.array_equal(out, want)
    print("%-60s want inf=%d got inf=%d %s" % (label, winf, inf, "ok" if ok else "MISMATCH"))
    assert inf == winf, label
    assert np.array_equal(out, want), label
    assert not (winf and out.any()), label


@pytest.mark.parametrize("pipe", PIPELINE_NAMES)
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_a_opposite_pairs_in_one_bucket(gpu_ctx, oracle, api, curve, pipe):
    """A. P_j and -P_j with equal scalars, interleaved and in separate halves: every bucket sum is O, the result is O although
    every scalar is non-zero.  Random scalars; two repeated values in 64-entry tasks (a hot bucket per window on either fold tier:
    cancellation inside tasks, between task partials and in k_task_fold's trees); one digit in one window."""
    p = msm_pipeline(curve, pipe)
    n = p["n"]
    shift = p["offs"][min(7, len(p["offs"]) - 1)]
    task_len = gpu_ctx.get_option("msm_task_len")
    for arrangement in ("interleaved", "halves"):
        bases = hb = None
        for variant in ("random", "repeated", "aligned"):
            ks, sc = family_a(curve, n, arrangement, variant, shift, 10)
            if bases is None:
                hb = signed_multiples(curve, ks)
                bases = _resident(api, gpu_ctx, curve, p, hb)
            want, winf = msm_two_references(curve, hb, ks, sc, key=("A", curve, n, arrangement, variant, shift))
            assert winf == 1
            gpu_ctx.set_option("msm_task_len", 64 if variant == "repeated" else task_len)
            _check(bases, curve, want, winf, sc, "A %s %s %s %s" % (curve, pipe, arrangement, variant))
        bases.free()


@pytest.mark.parametrize("pipe", PIPELINE_NAMES)
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_b_cancellation_then_more(gpu_ctx, oracle, api, curve, pipe):
    """B. Family A, third copies (P, -P, P), duplicates (P, P) and fresh pairs, shuffled: accumulators and running sums pass
    through O, double, and must go on adding correctly; the result is a finite point."""
    p = msm_pipeline(curve, pipe)
    n = p["n"]
    for variant in ("random", "repeated"):
        ks, sc = family_b(curve, n, variant)
        hb = signed_multiples(curve, ks)
        want, winf = msm_two_references(curve, hb, ks, sc, key=("B", curve, n, variant))
        assert winf == 0
        bases = _resident(api, gpu_ctx, curve, p, hb)
        if variant == "repeated":
            gpu_ctx.set_option("msm_task_len", 64)
        _check(bases, curve, want, winf, sc, "B %s %s %s" % (curve, pipe, variant))
        bases.free()


@pytest.mark.parametrize("pipe", PIPELINE_NAMES)
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_c_s_and_r_minus_s_on_one_base(gpu_ctx, oracle, api, curve, pipe):
    """C. Every base twice, with s and r - s: no bucket cancels, the total does -- in the last additions of the reduction
    (k_sum_parts, k_sum_final_coop) or in host_horner."""
    p = msm_pipeline(curve, pipe)
    n = p["n"]
    for arrangement in ("interleaved", "halves"):
        ks, sc = family_c(curve, n, arrangement)
        hb = signed_multiples(curve, ks)
        want, winf = msm_two_references(curve, hb, ks, sc, key=("C", curve, n, arrangement))
        assert winf == 1
        bases = _resident(api, gpu_ctx, curve, p, hb)
        _check(bases, curve, want, winf, sc, "C %s %s %s" % (curve, pipe, arrangement))
        bases.free()


@pytest.mark.parametrize("pipe", PIPELINE_NAMES[:3])
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_d_two_contribution_probes(gpu_ctx, oracle, api, curve, pipe):
    """D. All scalars zero but two or three: exactly two non-zero contributions X and -X (then X and X) that first meet at a
    chosen node -- one lane's running sum, the LDS trees, different workgroups, the final sum, neighbouring windows
    (host_horner, or one bucket through two window tables), two pieces (helpers.family_d).  One base vector and one
    precompute() per pipeline; the pipelines whose window layout the probes can aim at (not the cost model's tables)."""
    p = msm_pipeline(curve, pipe)
    n = p["n"]
    ks, probes, pieces = family_d(curve, n, p["c"], p["offs"])
    hb = signed_multiples(curve, ks)
    bases = _resident(api, gpu_ctx, curve, p, hb)
    failed = []
    for label, sc in probes + pieces:
        if label == pieces[0][0]:
            gpu_ctx.set_option("msm_max_piece_log", n.bit_length() - 2)         # two pieces of n / 2 pairs
        want, winf = msm_two_references(curve, hb, ks, sc)
        out, inf = bases.msm(scalar_limbs(curve, n, sc))
        ok = inf == winf and np.array_equal(out, want) and not (winf and out.any())
        print("D %s %s %-44s want inf=%d got inf=%d %s" % (curve, pipe, label, winf, inf, "ok" if ok else "MISMATCH"))
        if not ok:
            failed.append(label)
    bases.free()
    assert not failed, failed


@pytest.mark.parametrize("pipe", PIPELINE_NAMES)
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_e_random_signs_small_scalars(gpu_ctx, oracle, api, curve, pipe):
    """E. Bases +-G at random, one small digit each: ~64 entries per bucket whose partial sums walk through O, bucket sums that
    are small multiples of G of both signs and O, running sums and tree nodes that repeat and cancel.  A seeded sweep of scalar
    vectors on one base vector."""
    p = msm_pipeline(curve, pipe)
    n = p["n"]
    max_digit = min(1 << 11, n // 64)
    ks, vectors = family_e(curve, n, max_digit, E_VECTORS)
    hb = signed_multiples(curve, ks)
    bases = _resident(api, gpu_ctx, curve, p, hb)
    for v, sc in enumerate(vectors):
        want, winf = msm_two_references(curve, hb, ks, sc, key=("E", curve, n, max_digit, v))
        _check(bases, curve, want, winf, sc, "E %s %s vector %d" % (curve, pipe, v))
    bases.free()


@pytest.mark.parametrize("pipe", PIPELINE_NAMES)
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_f_unstructured_bases_with_holes(gpu_ctx, oracle, api, curve, pipe):
    """F. pm_bases_upload of multiples in random order with points at infinity, exact and negated duplicates: the download
    round trip, the per-window MSM, the pipeline's own MSM and an offset sub-range."""
    p = msm_pipeline(curve, pipe)
    n = p["n"]
    ks, sc = family_f(curve, n)
    hb = signed_multiples(curve, ks)
    want, winf = msm_two_references(curve, hb, ks, sc, key=("F", curve, n))
    for k, v in p["options"].items():
        gpu_ctx.set_option(k, v)
    bases = api.Bases.upload(gpu_ctx, curve, hb)
    assert len(bases) == n and np.array_equal(bases.download(), hb)
    _check(bases, curve, want, winf, sc, "F %s %s plain" % (curve, pipe))
    if p["tables"]:
        bases.precompute()
        assert np.array_equal(bases.download(), hb)
        _check(bases, curve, want, winf, sc, "F %s %s tables" % (curve, pipe))
    lo, cnt = n // 5 + 3, n // 2 + 1
    assert np.array_equal(bases.download(lo, cnt), hb[lo:lo + cnt])
    want, winf = msm_two_references(curve, hb[lo:lo + cnt], ks[lo:lo + cnt], sc[lo:lo + cnt], key=("F-sub", curve, n))
    _check(bases, curve, want, winf, sc[lo:lo + cnt], "F %s %s sub-range" % (curve, pipe), offset=lo)
    bases.free()


@pytest.mark.parametrize("curve", CURVE_LIST)
def test_g_host_sums_and_tiny_msm(gpu_ctx, oracle, curve):
    """G. pm_g1_sum (the dense host formulas host_horner and the rank combine rely on) and the host-stride pm_msm_g1 on
    [P, -P], [P, P], [O, P, -P, O], [P, -P, Q], ...: scalars 1, one repeated scalar, and scalars that cancel a duplicate."""
    r = CURVES[curve].r
    for label, ks in FAMILY_G:
        hb = signed_multiples(curve, ks)
        ones = [1] * len(ks)
        want, winf = msm_two_references(curve, hb, ks, ones)
        for infs in (None, [int(k == 0) for k in ks]):
            out, inf = gpu_ctx.g1_sum(curve, hb, infs)
            assert inf == winf and np.array_equal(out, want) and not (winf and out.any()), label
        ref, rinf = oracle.g1_sum(curve, hb, [int(k == 0) for k in ks])
        assert rinf == winf and (rinf or np.array_equal(ref, want)), label
        for sc in (ones, [0x1234567] * len(ks), [(r - 7 if i % 2 else 7) for i in range(len(ks))]):
            want, winf = msm_two_references(curve, hb, ks, sc)
            out, inf = gpu_ctx.msm(curve, hb, scalar_limbs(curve, len(ks), sc))
            print("G %s %-14s want inf=%d got inf=%d" % (curve, label, winf, inf))
            assert inf == winf and np.array_equal(out, want) and not (winf and out.any()), (label, sc[:2])
