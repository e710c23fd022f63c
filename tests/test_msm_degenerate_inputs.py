"""CPU: the inputs and the references of test_gpu_msm_degenerate.py, without a GPU.

Every input family of that file is generated here at its real size (tests/helpers.py: family_a ... family_f, FAMILY_G, on the
pipelines of msm_pipeline) and its two expectations are compared with each other: the C++ restatement's Pippenger with complete
additions (oracle.msm) and the closed form (sum s_i k_i mod r) G (oracle.g1_mul; oracle/pyref big integers once per family).
Also what the families CLAIM: opposite pairs carry equal scalars, the cancelling families sum to O with every scalar non-zero,
the "and then more" ones do not, a probe that doubles gives exactly 2 X.  This must pass before the GPU file means anything."""
import numpy as np
import pytest

from helpers import (FAMILY_G, PIPELINE_NAMES, family_a, family_b, family_c, family_d, family_e, family_f, fr_mont_limbs, msm_closed_form,
                     msm_pipeline, msm_two_references, signed_multiples)
from oracle import cpp_oracle as CO
from oracle.pyref import fields as F
from oracle.pyref.fields import CURVES

CURVE_LIST = ["bls12_381", "bn254"]
E_VECTORS = 12


def _pyref_agrees(curve, ks, scalars, want, winf):
    """the closed form once more, on Python integers alone"""
    c = CURVES[curve]
    _, _, total = msm_closed_form(curve, ks, scalars)
    pt = F.g1_mul(c, c.g1, total) if total else None
    assert (pt is None) == bool(winf)
    assert CO.g1_from_mont_limbs(curve, want, [winf])[0] == pt


@pytest.mark.parametrize("curve", CURVE_LIST)
def test_signed_multiples_are_the_points_they_claim(curve):
    c = CURVES[curve]
    ks = [1, -1, 2, -2, 0, 7, -7, 300, -300, 1 << 14, -(1 << 17)] + list(range(-20, 21))
    hb = signed_multiples(curve, ks)
    pts = CO.g1_from_mont_limbs(curve, hb)
    for k, row, pt in zip(ks, hb, pts):
        assert CO.g1_is_on_curve(curve, row)
        want = None if k == 0 else F.g1_mul(c, c.g1, abs(k))
        assert pt == (F.g1_neg(c, want) if k < 0 else want), k
    big = signed_multiples(curve, np.arange(-100, 101))                  # the table path (more than 64 magnitudes)
    assert np.array_equal(big[100:], signed_multiples(curve, list(range(0, 101)))) and not big[100].any()
    assert CO.g1_from_mont_limbs(curve, big[:1])[0] == F.g1_neg(c, F.g1_mul(c, c.g1, 100))
    assert np.array_equal(fr_mont_limbs(curve, [0, 1, c.r - 1, 12345]), CO.fr_to_mont_limbs(curve, [0, 1, c.r - 1, 12345]))


@pytest.mark.parametrize("pipe", PIPELINE_NAMES)
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_families_a_b_c_reference_equals_closed_form(curve, pipe):
    p = msm_pipeline(curve, pipe)
    n, r = p["n"], CURVES[curve].r
    shift, bits = p["offs"][min(7, len(p["offs"]) - 1)], 10
    for arrangement in ("interleaved", "halves"):
        hb = None
        for variant in ("random", "repeated", "aligned"):
            ks, sc = family_a(curve, n, arrangement, variant, shift, bits)
            hb = signed_multiples(curve, ks) if hb is None else hb
            assert len(ks) == n and all(0 < s < r for s in sc)
            if arrangement == "interleaved":
                assert np.array_equal(ks[0::2], -ks[1::2]) and sc[0::2] == sc[1::2]
            else:
                assert np.array_equal(ks[:n // 2], -ks[n // 2:]) and sc[:n // 2] == sc[n // 2:]
            if variant == "aligned":
                assert all(s >> shift << shift == s and s >> shift < 1 << bits for s in sc)
            want, winf = msm_two_references(curve, hb, ks, sc, key=("A", curve, n, arrangement, variant, shift))
            assert winf == 1 and not want.any()
        ks, sc = family_c(curve, n, arrangement)
        assert (ks > 0).all() and all(0 < s < r for s in sc)
        want, winf = msm_two_references(curve, signed_multiples(curve, ks), ks, sc, key=("C", curve, n, arrangement))
        assert winf == 1
    for variant in ("random", "repeated"):
        ks, sc = family_b(curve, n, variant)
        assert len(ks) == n == len(sc) and (ks == 0).sum() >= 1
        want, winf = msm_two_references(curve, signed_multiples(curve, ks), ks, sc, key=("B", curve, n, variant))
        assert winf == 0
        _pyref_agrees(curve, ks, sc, want, winf)


@pytest.mark.parametrize("pipe", PIPELINE_NAMES[:3])
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_family_d_reference_equals_closed_form(curve, pipe):
    p = msm_pipeline(curve, pipe)
    n, c, r = p["n"], p["c"], CURVES[curve].r
    ks, probes, pieces = family_d(curve, n, c, p["offs"])
    hb = signed_multiples(curve, ks)
    assert len({label for label, _ in probes + pieces}) == len(probes) + len(pieces)
    seen = set()
    for label, sc in probes + pieces:
        assert all(0 < s < r for s in sc.values())
        want, winf = msm_two_references(curve, hb, ks, sc)
        kind = label.split(" ")[0]
        seen.add(kind)
        assert winf == int("cancel" in kind and not kind.endswith("more")), label
        if "double" in kind:                    # X + X: twice the first contribution
            i0 = min(sc)
            assert msm_closed_form(curve, ks, sc)[2] == 2 * int(ks[i0]) * sc[i0] % r, label
    assert {"meet-cancel-2x-G", "meet-double-2x+G", "meet-cancel-2G", "meet-double+2G", "cross-cancel", "cross-double", "cross-same-point-cancel",
            "cross-same-point-double", "lane-opposite", "lane-equal", "pieces-cancel", "pieces-double", "pieces-cancel-then-more"} == seen
    _pyref_agrees(curve, ks, probes[1][1], *msm_two_references(curve, hb, ks, probes[1][1]))
    # the meeting point sweeps every power of two up to half the bucket set
    ts = sorted({int(label.split("t=")[1].split(" ")[0]) for label, _ in probes if label.startswith("meet-cancel-2x-G")})
    assert ts == [1 << k for k in range(c - 1)]


@pytest.mark.parametrize("pipe", PIPELINE_NAMES)
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_families_e_f_reference_equals_closed_form(curve, pipe):
    p = msm_pipeline(curve, pipe)
    n = p["n"]
    max_digit = min(1 << 11, n // 64)
    ks, vectors = family_e(curve, n, max_digit, E_VECTORS)
    assert set(np.unique(ks)) == {-1, 1} and len(vectors) == E_VECTORS
    hb = signed_multiples(curve, ks)
    infs = 0
    for v, sc in enumerate(vectors):
        assert 1 <= min(sc) and max(sc) == max_digit
        want, winf = msm_two_references(curve, hb, ks, sc, key=("E", curve, n, max_digit, v))
        infs += winf
    assert infs < E_VECTORS
    _pyref_agrees(curve, ks, vectors[0], *msm_two_references(curve, hb, ks, vectors[0], key=("E", curve, n, max_digit, 0)))
    ks, sc = family_f(curve, n)
    hb = signed_multiples(curve, ks)
    holes, mags = int((ks == 0).sum()), np.abs(ks[ks != 0])
    assert holes >= n // 100 and len(mags) - len(np.unique(mags)) >= 2 * (n // 100) and (ks < 0).sum() >= n // 100
    assert list(np.sort(mags)[:8]) != list(mags[:8])                       # not in index order
    want, winf = msm_two_references(curve, hb, ks, sc, key=("F", curve, n))
    assert winf == 0
    _pyref_agrees(curve, ks, sc, want, winf)
    lo, cnt = n // 5 + 3, n // 2 + 1                                       # the offset sub-range the GPU test runs
    msm_two_references(curve, hb[lo:lo + cnt], ks[lo:lo + cnt], sc[lo:lo + cnt], key=("F-sub", curve, n))


@pytest.mark.parametrize("curve", CURVE_LIST)
def test_family_g_sums(curve):
    for label, ks in FAMILY_G:
        hb = signed_multiples(curve, ks)
        want, winf, total = msm_closed_form(curve, ks, [1] * len(ks))
        ref, rinf = CO.g1_sum(curve, hb, [int(k == 0) for k in ks])
        assert rinf == winf == int(sum(ks) == 0) and np.array_equal(ref if not rinf else np.zeros_like(ref), want), label
        msm_two_references(curve, hb, ks, [3] * len(ks))
