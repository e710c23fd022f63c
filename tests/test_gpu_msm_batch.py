"""GPU: pm_msm_g1_resident_batch -- many scalar rows against one resident base range in one call.

A batch of B rows runs the per-window pipeline over B * nwin bucket sets (msm.hip: msm_run_batch), recodes its digits over
(row, i) (k_digits_batch) and combines each row's window sums on the device (k_window_combine).  Every row is compared, bit for
bit, with the CPU oracle's MSM of that row and with the single-MSM entry point; shapes are the smallest at which each mechanism
can break: one pair, one row, a length below / across / above the 64-entry task and the 256-lane digit workgroup, more rows than
one combine workgroup's wave handles alone, the group split and the row-by-row fallback."""
import ctypes as ct

import numpy as np
import pytest

from helpers import rand_fr_limbs
from oracle.pyref.fields import CURVES

pytestmark = pytest.mark.gpu

CURVE_LIST = ["bls12_381", "bn254"]


@pytest.fixture(scope="module")
def api():
    from polymath_amd import api as _api
    return _api


def _rows(curve, batch, n, seed):
    return rand_fr_limbs(curve, batch * n, seed).reshape(batch, n, 4)


def _check_rows(oracle, curve, hb, rows, out, inf, label=""):
    assert out.shape == (len(rows), hb.shape[1]) and inf.shape == (len(rows),)
    for b, row in enumerate(rows):
        ref, rinf = oracle.msm(curve, hb, row, 8)
        assert inf[b] == rinf, (label, b)
        if rinf:
            assert not out[b].any(), (label, b)
        else:
            assert np.array_equal(out[b], ref), (label, b)


@pytest.mark.parametrize("curve", CURVE_LIST)
@pytest.mark.parametrize("n,batch", [(1, 1), (1, 5), (65, 3), (1000, 7), (4096, 33)])
def test_batch_rows_equal_oracle_and_single_msm(gpu_ctx, oracle, api, curve, n, batch):
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    hb = bases.download()
    rows = _rows(curve, batch, n, 9000 + 13 * n + batch)
    out, inf = bases.msm_batch(rows)
    _check_rows(oracle, curve, hb, rows, out, inf)
    for b in range(batch):
        one, oinf = bases.msm(rows[b])
        assert oinf == inf[b] and np.array_equal(one, out[b]), b
    bases.free()


def test_degenerate_rows_in_one_batch(gpu_ctx, oracle, api):
    """Rows whose window sums coincide, cancel or vanish (bases G, 2G, ...), between ordinary neighbours."""
    curve, n = "bls12_381", 1000
    r = CURVES[curve].r
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    hb = bases.download()
    rnd = _rows(curve, 4, n, 4242)
    s_int = [int(v) for v in np.random.default_rng(7).integers(1, 1 << 62, size=n)]
    s = oracle.fr_to_mont_limbs(curve, s_int)
    neg_s = oracle.fr_to_mont_limbs(curve, [r - v for v in s_int])
    ones = oracle.fr_to_mont_limbs(curve, [1] * n)
    minus_ones = oracle.fr_to_mont_limbs(curve, [r - 1] * n)
    single = np.zeros((n, 4), dtype=np.uint64)
    single[613] = oracle.fr_to_mont_limbs(curve, [0x1234567])[0]
    zero = np.zeros((n, 4), dtype=np.uint64)
    rows = np.stack([rnd[0], zero, rnd[1], rnd[1], s, neg_s, rnd[2], ones, minus_ones, single, rnd[3]])
    out, inf = bases.msm_batch(rows)
    _check_rows(oracle, curve, hb, rows, out, inf)
    assert inf[1] == 1 and not out[1].any()                                   # all-zero row
    assert inf[2] == inf[3] == 0 and np.array_equal(out[2], out[3])           # identical rows
    tot, tinf = api.g1_sum(curve, out[4:6], inf[4:6])                         # a row and its negation
    assert tinf == 1 and not tot.any()
    tot, tinf = api.g1_sum(curve, out[7:9], inf[7:9])                         # all ones and all r - 1
    assert tinf == 1 and not tot.any()
    bases.free()


def test_infinity_base_is_skipped_in_every_row(gpu_ctx, oracle, api):
    curve, n = "bls12_381", 300
    hb = oracle.g1_multiples(curve, n).copy()
    hb[0] = 0
    hb[77] = 0
    hb[n - 1] = 0
    bases = api.Bases.upload(gpu_ctx, curve, hb)
    rows = _rows(curve, 3, n, 515)
    rows[1, :, :] = 0
    rows[1, 77] = oracle.fr_to_mont_limbs(curve, [CURVES[curve].r - 1])[0]     # the whole weight of row 1 on O
    rows[2, 0] = rows[2, 77] = rows[2, n - 1] = oracle.fr_to_mont_limbs(curve, [CURVES[curve].r - 2])[0]
    out, inf = bases.msm_batch(rows)
    _check_rows(oracle, curve, hb, rows, out, inf)
    assert inf[1] == 1
    bases.free()


def test_sub_range_of_the_bases(gpu_ctx, oracle, api):
    curve, n, m = "bn254", 3000, 1500
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    hb = bases.download()
    rows = _rows(curve, 4, m, 616)
    out, inf = bases.msm_batch(rows, offset=777, length=m)
    _check_rows(oracle, curve, hb[777:777 + m], rows, out, inf)
    bases.free()


def test_group_split_and_row_by_row_fallback(gpu_ctx, oracle, api):
    """msm_max_piece_log = 12: 7 rows of 1000 pairs run as groups of 4 + 3; rows of 5000 pairs exceed one piece and run one by one."""
    curve = "bls12_381"
    bases = api.Bases.multiples(gpu_ctx, curve, 5000)
    hb = bases.download()
    before = gpu_ctx.get_option("msm_max_piece_log")
    try:
        for n, batch in ((1000, 7), (5000, 3)):
            rows = _rows(curve, batch, n, 717 + n)
            whole, winf = bases.msm_batch(rows, length=n)
            gpu_ctx.set_option("msm_max_piece_log", 12)
            split, sinf = bases.msm_batch(rows, length=n)
            gpu_ctx.set_option("msm_max_piece_log", before)
            assert np.array_equal(whole, split) and np.array_equal(winf, sinf), n
            _check_rows(oracle, curve, hb[:n], rows, split, sinf, n)
    finally:
        gpu_ctx.set_option("msm_max_piece_log", before)
    bases.free()


def test_precomputed_bases_give_the_same_points(gpu_ctx, oracle, api):
    curve, n = "bls12_381", 2000
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    hb = bases.download()
    rows = _rows(curve, 5, n, 818)
    plain, pinf = bases.msm_batch(rows)
    bases.precompute()
    tabled, tinf = bases.msm_batch(rows)
    assert np.array_equal(plain, tabled) and np.array_equal(pinf, tinf)
    _check_rows(oracle, curve, hb, rows, tabled, tinf)
    bases.free()


def test_device_resident_scalars(gpu_ctx, api):
    hip = ct.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ct.POINTER(ct.c_void_p), ct.c_size_t]
    hip.hipMemcpy.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_int]
    hip.hipFree.argtypes = [ct.c_void_p]
    curve, n, batch = "bn254", 700, 6
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    rows = _rows(curve, batch, n, 919)
    host, hinf = bases.msm_batch(rows)
    p = ct.c_void_p()
    assert hip.hipMalloc(ct.byref(p), rows.nbytes) == 0
    assert hip.hipMemcpy(p, rows.ctypes.data_as(ct.c_void_p), rows.nbytes, 1) == 0   # hipMemcpyHostToDevice
    dev, dinf = bases.msm_batch(None, length=n, device_ptr=p.value, batch=batch)
    hip.hipFree(p)
    assert np.array_equal(host, dev) and np.array_equal(hinf, dinf)
    bases.free()


def test_errors_empty_batch_and_recovery(gpu_ctx, oracle, api):
    curve, n = "bls12_381", 64
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    hb = bases.download()
    with pytest.raises(api.PolymathError) as single:
        bases.msm(rand_fr_limbs(curve, n + 1, 1))
    with pytest.raises(api.PolymathError) as batched:
        bases.msm_batch(_rows(curve, 3, n + 1, 2))
    assert batched.value.status == single.value.status == 2          # PM_ERR_LEN_MISMATCH
    with pytest.raises(api.PolymathError) as batched:
        bases.msm_batch(_rows(curve, 3, n, 2), offset=1)
    assert batched.value.status == 2
    out, inf = bases.msm_batch(np.zeros((0, n, 4), dtype=np.uint64))
    assert out.shape == (0, hb.shape[1]) and inf.shape == (0,)
    out, inf = bases.msm_batch(np.zeros((4, 0, 4), dtype=np.uint64))  # len == 0: every row is the identity
    assert out.shape == (4, hb.shape[1]) and not out.any() and list(inf) == [1, 1, 1, 1]
    rows = _rows(curve, 3, n, 3)
    out, inf = bases.msm_batch(rows)                                  # the context still computes
    _check_rows(oracle, curve, hb, rows, out, inf)
    bases.free()


def test_timings_cover_the_batch(gpu_ctx, api):
    curve, n = "bls12_381", 500
    bases = api.Bases.multiples(gpu_ctx, curve, n)
    bases.msm_batch(_rows(curve, 4, n, 77))
    t = gpu_ctx.timings()
    assert t["msm_total"] > 0 and t["msm_sort"] > 0 and t["msm_accumulate"] > 0 and t["msm_reduce"] > 0
    bases.free()
