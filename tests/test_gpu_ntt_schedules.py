"""The transform on its own, at every pass schedule ntt_run_batch (polymath_amd/csrc/ntt.hip) can select, as batched rows, through
the device-buffer entry points, and across evictions of the context's twiddle-table slots.  All arithmetic is integer: every
comparison is exact equality, in both directions (forward, and inverse with its 1/n).

ntt_run_batch picks its kernels from log_n alone (one row per domain):

| log_n | path | stages per pass | workgroup / tile | log_cols per pass |
|---|---|---|---|---|
| 1-8 | dense (k_bitrev + k_ntt_pass [+ k_scale]) | one pass of log_n | 256 | 0 |
| 9, 10 | dense | 8 + 1, 8 + 2 | 256 | 0, 3 |
| 11, 12, 13 | reduced-radix tiles | 6+5, 6+6, 7+6 | TH 256 / 2^10 | 4,5 / 4,4 / 3,4 |
| 14, 15, 16 | tiles | 7+7, 8+7, 8+8 | TH 256 | 3,3 / 2,3 / 2,2 |
| 17, 18 | tiles | 9+8, 9+9 | TH 512 / 2^11 | 2,3 / 2,2 |
| 19, 20, 21 | tiles | 7+6+6, 7+7+6, 7+7+7 | TH 256 | 3,4,4 / 3,3,4 / 3,3,3 |
| 22, 23, 24 | tiles | 8+7+7, 8+8+7, 8+8+8 | TH 256 | 2,3,3 / 2,2,3 / 2,2,2 |
| 25, 26, 27 | tiles | 9+8+8, 9+9+8, 9+9+9 | TH 512 | 2,3,3 / 2,2,3 / 2,2,2 |
| 28 | tiles | 7+7+7+7 (the only four-pass schedule) | TH 256 | 3,3,3,3 |

test_gpu_parity.py compares log_n 1, 4, 7, 8, 9, 11, 12, 13, 16-20 (and 21 on BN254) with the oracle; this file adds the rest:
2, 3, 5, 6, 10, 14, 15 and 22, 23, 24 against the oracle, 26, 27, 28 against closed forms and big-integer sums on the device,
the batched rows (pm_ntt_batch_device, row_stride == n and > n) on dense one / two passes, the first tile domain, 7+7, 8+7, 8+8,
the TH 512 tile and three passes, pm_ntt_device against pm_ntt, and a context whose 8 twiddle slots are all evicted and change
their record type (dense Fr <-> Tw28) before the first keys come back.

Wall times of the two heavy tests on an MI355X box (recorded, not asserted; oracle.ntt on 8 threads included):
test_ntt_full_size_vs_oracle: 1.3 s (BLS12-381 2^22), 2.8 s (2^23), 5.4 s (2^24), 4.2 s (BN254 2^23) -- both directions at every
size, 2^24 included.  test_ntt_full_size_above_2p24_on_the_device: 2.4 s (2^26), 3.0 s (2^27), 3.4 s (BN254 2^28), of which 0.3 /
0.4 / 0.6 s are the transforms and checks inside the child and the rest is its start-up (importing torch).
"""
import ctypes as ct
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from helpers import rand_fr_limbs
from oracle.pyref.fields import CURVES

pytestmark = pytest.mark.gpu

CURVE_LIST = ["bls12_381", "bn254"]
SENTINEL = 0x5A5A5A5A5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    from polymath_amd import api as _api
    return _api


# ------------------------------------------------------------------------------------ a. sizes never compared with the oracle
@pytest.mark.parametrize("curve", CURVE_LIST)
@pytest.mark.parametrize("log_n", [2, 3, 5, 6, 10, 14, 15])
def test_ntt_remaining_sizes_vs_oracle(gpu_ctx, oracle, curve, log_n):
    """Dense single passes shorter than the tile (2, 3, 5, 6), dense 8 + 2 with 8-column tiles in the second pass (10), and the
    tile schedules 7+7 and 8+7 (14, 15)."""
    a = rand_fr_limbs(curve, 1 << log_n, 300 + log_n)
    for inverse in (False, True):
        assert np.array_equal(gpu_ctx.ntt(curve, a, log_n, inverse), oracle.ntt(curve, a, log_n, inverse, 8)), (log_n, inverse)


# ------------------------------------------------------------------------------------ b. full-size schedules against the oracle
@pytest.mark.parametrize("curve,log_n", [("bls12_381", 22), ("bls12_381", 23), ("bls12_381", 24), ("bn254", 23)])
def test_ntt_full_size_vs_oracle(gpu_ctx, oracle, curve, log_n):
    """The three-pass schedules with 8-stage passes, 8+7+7, 8+8+7 and 8+8+8, on random input against the oracle's transform, both
    directions at every size."""
    t0 = time.perf_counter()
    a = rand_fr_limbs(curve, 1 << log_n, 400 + log_n)
    for inverse in (False, True):
        got = gpu_ctx.ntt(curve, a, log_n, inverse)
        want = oracle.ntt(curve, a, log_n, inverse, 8)
        print("full size %s 2^%d inverse=%d: %.1f s since the start of the test" % (curve, log_n, inverse, time.perf_counter() - t0))
        assert np.array_equal(got, want), (log_n, inverse)


# ------------------------------------------------------------------------------------ c. schedules above 2^24
@pytest.mark.parametrize("curve,log_n", [("bls12_381", 26), ("bls12_381", 27), ("bn254", 28)])
def test_ntt_full_size_above_2p24_on_the_device(curve, log_n):
    """9+9+8, 9+9+9 (TH 512) and the only four-pass schedule, 7+7+7+7 at BN254's largest domain, through pm_ntt_device on torch
    tensors: no host array of the domain's size exists.  Run by tests/ntt_device_child.py in a process of its own (torch's HIP
    runtime has to be loaded before the library's, which this session can no longer do) on a context of its own, closed at the
    end: at 2^28 the twiddle tables are about 19 GB, the data and the out-of-place temporary 16 GB more.  Per size, checked on the
    device: a constant input c gives [n c, 0, ..., 0]; the inverse of c e_0 is c / n everywhere; 16 non-zero entries (0, 1, n/2,
    n - 1 and 12 random positions) give sum_j v_j w^(jk) at k = 0, 1, n/2, n - 1 and 60 random k (Python big integers; with w^-1
    and 1/n for the inverse); a dense random input comes back from forward + inverse and is changed by forward.
    (The limbs are taken as field elements as they stand: the transform is linear and its products are Montgomery products with
    Montgomery-form twiddles, so sum_j X_j w^(jk) holds for the stored integers.)
    Skipped only when hipMemGetInfo reports less free memory than the size needs (40 GiB at 2^28, half of it per size below)."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ntt_device_child.py"), curve, str(log_n)], capture_output=True, text=True,
                         cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    if "skip" in res:
        pytest.skip(res["skip"])
    print("above 2^24 %s 2^%d: %.1f s in the child" % (curve, log_n, res["wall_s"]))
    assert len(res["checks"]) == 7 and all(res["checks"].values()), res["checks"]


# ------------------------------------------------------------------------------------ d. batched rows
# Device buffers of the batched and the device-pointer tests: hipMalloc / hipMemcpy of the HIP runtime the library has loaded.
_hip = None


def _hiprt():
    global _hip
    if _hip is None:
        _hip = ct.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [ct.POINTER(ct.c_void_p), ct.c_size_t]
        _hip.hipMemcpy.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_int]
        _hip.hipFree.argtypes = [ct.c_void_p]
    return _hip


class DeviceArray:
    """A host uint64 array copied to a device allocation of the same size; .host() copies it back, .free() releases it."""

    def __init__(self, arr):
        self.shape, self.nbytes = arr.shape, arr.nbytes
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        p = ct.c_void_p()
        assert _hiprt().hipMalloc(ct.byref(p), self.nbytes) == 0
        self.ptr = p.value
        assert _hiprt().hipMemcpy(self.ptr, arr.ctypes.data, self.nbytes, 1) == 0      # hipMemcpyHostToDevice

    def host(self):
        out = np.empty(self.shape, dtype=np.uint64)
        assert _hiprt().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0      # hipMemcpyDeviceToHost
        return out

    def free(self):
        assert _hiprt().hipFree(self.ptr) == 0
        self.ptr = None


BATCH_ROWS = 5
_batch_refs = {}


def _batch_reference(ctx, oracle, curve, log_n):
    """Five random rows of one domain, ctx.ntt of every row alone in both directions (computed once per domain and left
    unchanged), and the oracle's transform of rows 0, 1 and 4: the first and the last row of the 1-, 2- and 5-row cases."""
    key = (curve, log_n)
    if key not in _batch_refs:
        n = 1 << log_n
        inp = rand_fr_limbs(curve, BATCH_ROWS * n, 500 + log_n).reshape(BATCH_ROWS, n, 4)
        single = {inv: np.stack([ctx.ntt(curve, inp[b], log_n, inv) for b in range(BATCH_ROWS)]) for inv in (False, True)}
        orc = {(inv, b): oracle.ntt(curve, inp[b], log_n, inv, 8) for inv in (False, True) for b in (0, 1, BATCH_ROWS - 1)}
        _batch_refs[key] = (inp, single, orc)
    return _batch_refs[key]


def _run_batch(ctx, curve, log_n, inverse, inp, rows, stride):
    """[rows][stride] device buffer filled with the sentinel, the rows' inputs written, one pm_ntt_batch_device call -> the
    buffer, copied back, as [rows, stride, 4]."""
    n = 1 << log_n
    buf = np.full((rows, stride, 4), SENTINEL, dtype=np.uint64)
    buf[:, :n] = inp[:rows]
    d = DeviceArray(buf)
    try:
        ctx.ntt_batch_device(curve, d.ptr, log_n, inverse, rows, stride)
        return d.host()
    finally:
        d.free()


@pytest.mark.parametrize("curve,log_n", [("bls12_381", l) for l in (7, 10, 11, 14, 15, 16, 17, 19)] + [("bn254", 11), ("bn254", 17)])
def test_ntt_batch_device_rows_and_strides(gpu_ctx, oracle, curve, log_n):
    """pm_ntt_batch_device with 1, 2 and 5 rows at row_stride n and n + 3, both directions: every row equals ctx.ntt of that row
    alone, row 0 and the last row equal the oracle's transform, and the three padding elements after every row still hold the
    sentinel.  With a stride above n the first tile pass reads with the caller's stride and writes the temporary with stride n,
    and the last pass does the reverse, so a pass that offsets one side by the other's stride mixes rows exactly here."""
    n = 1 << log_n
    inp, single, orc = _batch_reference(gpu_ctx, oracle, curve, log_n)
    for rows in (1, 2, BATCH_ROWS):
        for stride in (n, n + 3):
            for inverse in (False, True):
                out = _run_batch(gpu_ctx, curve, log_n, inverse, inp, rows, stride)
                tag = (curve, log_n, rows, stride, inverse)
                bad = [b for b in range(rows) if not np.array_equal(out[b, :n], single[inverse][b])]
                assert not bad, (tag, "rows that differ from the single transform", bad)
                assert np.array_equal(out[:, n:], np.full((rows, stride - n, 4), SENTINEL, dtype=np.uint64)), (tag, "padding overwritten")
                for b in {0, rows - 1}:
                    assert np.array_equal(out[b, :n], orc[(inverse, b)]), (tag, b)


def test_ntt_batch_device_error_paths(gpu_ctx, oracle, api):
    """rows == 0 is PM_OK and touches nothing; rows == 65536 and row_stride == n - 1 are PM_ERR_INVALID_ARG; a domain above the
    field's two-adicity is PM_ERR_DOMAIN_TOO_LARGE (3); none of them writes the buffer, and after each the same context still
    transforms a batch correctly."""
    log_n, n, rows = 11, 1 << 11, 2
    for curve in CURVE_LIST:
        inp, single, _ = _batch_reference(gpu_ctx, oracle, curve, log_n)
        before = np.full((rows * n, 4), SENTINEL, dtype=np.uint64)
        buf = DeviceArray(before)

        def status(lg, nrows, stride):
            return gpu_ctx.L.pm_ntt_batch_device(gpu_ctx.h, api.CURVE_IDS[curve], ct.c_void_p(buf.ptr), lg, 0, nrows, stride)

        def still_works():
            assert np.array_equal(buf.host(), before)
            for inverse in (False, True):
                out = _run_batch(gpu_ctx, curve, log_n, inverse, inp, rows, n + 3)
                assert np.array_equal(out[:, :n], single[inverse][:rows])
                assert np.array_equal(out[:, n:], np.full((rows, 3, 4), SENTINEL, dtype=np.uint64))

        try:
            assert status(log_n, 0, n) == 0
            still_works()
            assert status(log_n, 65536, n) == 1
            still_works()
            assert status(log_n, rows, n - 1) == 1
            still_works()
            too_large = CURVES[curve].two_adicity + 1
            assert status(too_large, 1, 1 << too_large) == 3
            with pytest.raises(api.PolymathError) as e:
                gpu_ctx.ntt_batch_device(curve, buf.ptr, too_large, False, 1, 1 << too_large)
            assert e.value.status == 3
            still_works()
        finally:
            buf.free()


# ------------------------------------------------------------------------------------ e. pm_ntt_device == pm_ntt
@pytest.mark.parametrize("curve", CURVE_LIST)
@pytest.mark.parametrize("log_n", [1, 10, 11, 17])
def test_ntt_device_equals_ntt(gpu_ctx, curve, log_n):
    a = rand_fr_limbs(curve, 1 << log_n, 600 + log_n)
    for inverse in (False, True):
        x = DeviceArray(a)
        try:
            gpu_ctx.ntt_device(curve, x.ptr, log_n, inverse)
            assert np.array_equal(x.host(), gpu_ctx.ntt(curve, a, log_n, inverse)), (log_n, inverse)
        finally:
            x.free()


# ------------------------------------------------------------------------------------ f. twiddle-table reuse
TW_SLOTS = 8
TW_KEYS = [("bls12_381", 3), ("bls12_381", 11), ("bn254", 10), ("bn254", 12), ("bls12_381", 9), ("bls12_381", 13), ("bn254", 5),
           ("bn254", 11), ("bls12_381", 10), ("bls12_381", 12)]
# With 8 slots evicted in turn, keys that alternate dense / tile keep meeting a slot of their own record type: after the ten keys
# and the three revisits five slots have been evicted and none has changed its type.  Eight further keys, alternating the other way
# round (the next victim holds a tile table, the first of them is dense), evict every slot once more into the other type.
TW_KEYS_RETYPE = [("bn254", 4), ("bls12_381", 14), ("bls12_381", 6), ("bn254", 13), ("bn254", 8), ("bn254", 14), ("bls12_381", 7),
                  ("bls12_381", 15)]
TW_VISITS = TW_KEYS + TW_KEYS[:3] + TW_KEYS_RETYPE + TW_KEYS[:3]


def _lru_model(visits):
    """What the sequence does to the slots under the policy of twiddles_slot (a hit refreshes the stamp, a miss takes the first
    slot with the smallest stamp): per slot, the number of evictions and of changes between dense (log_n < 11) and tile records."""
    slots = [dict(key=None, stamp=0, evicted=0, retyped=0) for _ in range(TW_SLOTS)]
    for clock, key in enumerate(visits, 1):
        hit = [s for s in slots if s["key"] == key]
        s = hit[0] if hit else min(slots, key=lambda t: t["stamp"])
        if not hit and s["key"] is not None:
            s["evicted"] += 1
            s["retyped"] += (s["key"][1] >= 11) != (key[1] >= 11)
        s["key"], s["stamp"] = key, clock
    return slots


def test_ntt_twiddle_slots_evicted_retyped_and_revisited(oracle, api):
    """A context has 8 TwiddleCache slots, least recently used evicted, keyed by (curve, log_n); a slot's internal-form tables hold
    dense Fr records for dense domains and Tw28 records for tile domains.  On a fresh context: ten distinct keys, dense and tile
    domains in turn, the first three again (evicted by then, or about to be), eight more keys that put a dense table where a tile
    table was and the reverse in every slot, and the first three a third time.  Every output equals the oracle's, both directions,
    first visit and revisit alike."""
    assert len(set(TW_KEYS + TW_KEYS_RETYPE)) == 18
    assert all(s["evicted"] >= 2 and s["retyped"] >= 1 for s in _lru_model(TW_VISITS))
    ctx = api.Context(0)
    try:
        for visit, (curve, log_n) in enumerate(TW_VISITS):
            a = rand_fr_limbs(curve, 1 << log_n, 700 + visit)
            for inverse in (False, True):
                assert np.array_equal(ctx.ntt(curve, a, log_n, inverse), oracle.ntt(curve, a, log_n, inverse, 8)), (visit, curve, log_n, inverse)
    finally:
        ctx.close()
