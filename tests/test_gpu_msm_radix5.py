"""GPU: the window-table MSM on radix 5*2^a (csrc/radix.cuh; forced with table_window_bits = 500 + windows), against oracle/cpp and
the closed form (helpers.msm_two_references), both curves, at the smallest shapes that reach the new paths:

  2^13 pairs, 16 windows of radix 5*2^14: 40 960 buckets -- more than one sort region and not whole ones (padded to two), the
       two-level reduction on a bucket count that is no power of two;
  2^14 pairs, 14 windows of radix 5*2^16: 163 840 buckets = 5 regions, the three-level sort on a region count that is no power of two.

(The level-0 fan-in K0 = ceil(buckets / 2^17) leaves 4 only above 2^19 buckets: K0 = 10 and 40, with level 1's double-and-add, run in
test_gpu_prove_radix5.py.)  Scalars: the hostile list of the CPU self-test (tests/native/radix_selftest.cpp) padded with random
ones; one value repeated on every base (one hot bucket per window: k_task_fold); bases at infinity."""
import numpy as np
import pytest

from helpers import msm_two_references, scalar_limbs, signed_multiples
from oracle.pyref.fields import CURVES

pytestmark = pytest.mark.gpu

CURVE_LIST = ["bls12_381", "bn254"]
SHAPES = {"16x5*2^14": (1 << 13, 16, 14), "14x5*2^16": (1 << 14, 14, 16)}       # pairs, windows, shift


@pytest.fixture(scope="module")
def api():
    from polymath_amd import api as _api
    return _api


def _hostile_scalars(curve, n, W, a):
    import random
    r = CURVES[curve].r
    R = 5 << a
    H = R // 2
    out = [0, 1, r - 1, (r - 1) // 2, ((1 << 255) - 19) % r]
    for j in range(W):
        out += [R ** j, R ** j + 1, R ** j - 1, H * R ** j + 1, H * R ** j - 1]
    top = (r - 1) // R ** (W - 1) - 1
    for dig in (H + 1, R - 1):         # a carry through every window; every digit at its largest (the top one held below r)
        out.append(sum(dig * R ** j for j in range(W - 1)) + min(dig, top) * R ** (W - 1))
    out = [s % r for s in out]
    rng = random.Random("radix5 %s %d %d" % (curve, W, a))
    return out + [rng.randrange(r) for _ in range(n - len(out))]


def _check(bases, curve, hb, ks, sc, label, key):
    want, winf = msm_two_references(curve, hb, ks, sc, key=key)
    out, inf = bases.msm(scalar_limbs(curve, len(sc), sc))
    print("%-60s want inf=%d got inf=%d" % (label, winf, inf))
    assert inf == winf and np.array_equal(out, want) and not (winf and out.any()), label


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_radix5_msm_vs_oracle(gpu_ctx, oracle, api, curve, shape):
    n, W, a = SHAPES[shape]
    r = CURVES[curve].r
    fits = lambda s: (r - 1) // (5 << s) ** (W - 1) + 1 <= (5 << s) // 2
    assert fits(a) and not fits(a - 1)                          # a = the planner's shift for W windows
    gpu_ctx.set_option("table_window_bits", 500 + W)            # restored by conftest
    ks = list(range(1, n + 1))
    hb = signed_multiples(curve, ks)
    bases = api.Bases.upload(gpu_ctx, curve, hb)
    bases.precompute()
    _check(bases, curve, hb, ks, _hostile_scalars(curve, n, W, a), "hostile %s %s" % (curve, shape), ("r5-hostile", curve, shape))
    # one value on every base: every window's entries in one bucket, folded by k_task_fold (64-entry tasks: both fold tiers)
    gpu_ctx.set_option("msm_task_len", 64)
    same = (0x1234567 * (5 << a) ** (W - 1) + 0x89ABCDEF0123456789) % r
    _check(bases, curve, hb, ks, [same] * n, "repeated %s %s" % (curve, shape), ("r5-same", curve, shape))
    bases.free()


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_radix5_msm_bases_at_infinity(gpu_ctx, oracle, api, curve, shape):
    n, W, a = SHAPES[shape]
    gpu_ctx.set_option("table_window_bits", 500 + W)
    ks = [0 if i % 7 == 3 or i < 5 or i >= n - 3 else (-(i + 1) if i % 11 == 0 else i + 1) for i in range(n)]
    hb = signed_multiples(curve, ks)
    bases = api.Bases.upload(gpu_ctx, curve, hb)
    bases.precompute()
    assert np.array_equal(bases.download(), hb)
    _check(bases, curve, hb, ks, _hostile_scalars(curve, n, W, a), "infinity %s %s" % (curve, shape), ("r5-inf", curve, shape))
    lo, cnt = n // 5 + 3, n // 2 + 1                            # an offset sub-range (tb.base_index)
    sc = _hostile_scalars(curve, cnt, W, a)
    want, winf = msm_two_references(curve, hb[lo:lo + cnt], ks[lo:lo + cnt], sc, key=("r5-inf-sub", curve, shape))
    out, inf = bases.msm(scalar_limbs(curve, cnt, sc), offset=lo)
    assert inf == winf and np.array_equal(out, want) and not (winf and out.any())
    bases.free()
