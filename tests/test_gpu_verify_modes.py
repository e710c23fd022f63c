"""GPU: pm_verify_batch2 in all four combinations of pairing in {host, device} x challenges in {host, device}, at the smallest counts
where the sum tree has padding: 1 (depth 0), 3 (padded 4) and 5 (padded 8).  What a wrong hand-over between the verifier's stages
(csrc/verify_batch.hip) would break: the four combinations must agree with each other and, proof by proof, with pm_host_verify.

Per curve and count, five batches of Merlin proofs from tests/verify_helpers.py: all valid; a(x1) + 1 in the last proof (the
neighbour of the padding); a moved point in proof 0; a(x1) = r in the middle proof; every proof with a(x1) = r.  One fixed seed.
The reference verdicts are computed once per distinct proof (eight pm_host_verify calls a curve that reach a pairing)."""
import ctypes as ct

import numpy as np
import pytest

from verify_helpers import CURVES2, G1N, _bound, _ctx, _host_verdict, _key, _moved_point, _plus_one, _proofs, _run

pytestmark = pytest.mark.gpu

SEED = bytes(range(7, 39))
COMBOS = [(p, c) for p in ("host", "device") for c in ("host", "device")]
BATCHES = ("all valid", "a(x1) + 1", "a moved point", "a(x1) = r", "every proof malformed")
_WANT, _BATCHES = {}, {}


def _want(curve, item):
    key = (curve, tuple(item[0]), item[1])
    if key not in _WANT:
        _WANT[key] = _host_verdict(curve, "merlin", item)
    return _WANT[key]


def _a_is_r(curve, item, r):
    g1 = G1N[curve]
    return (item[0], item[1][:2 * g1] + r.to_bytes(32, "little") + item[1][2 * g1 + 32:])


def _batches(curve, count):
    if (curve, count) in _BATCHES:
        return _BATCHES[curve, count]
    r = _key(curve)["pm"]["merlin"].field.r
    valid = list(_proofs(curve, "merlin", count))
    out = {"all valid": valid}
    for name, k, alter in (("a(x1) + 1", count - 1, lambda it: _plus_one(curve, it, r)), ("a moved point", 0, lambda it: _moved_point(curve, it)),
                           ("a(x1) = r", count // 2, lambda it: _a_is_r(curve, it, r))):
        items = list(valid)
        items[k] = alter(items[k])
        out[name] = items
    out["every proof malformed"] = [_a_is_r(curve, it, r) for it in valid]
    assert tuple(out) == BATCHES
    _BATCHES[curve, count] = out
    return out


def _tap8(curve, count):
    """-> (status, elements) of pm_prove_tap(8)"""
    ctx = _ctx(curve)
    rows, n = np.zeros((count, 4, 4), dtype=np.uint64), ct.c_size_t(0)
    st = ctx.L.pm_prove_tap(ctx.h, 8, rows.ctypes.data_as(ct.POINTER(ct.c_uint64)), 4 * count, ct.byref(n))
    return st, n.value


@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("count", (1, 3, 5))
@pytest.mark.parametrize("curve", CURVES2)
def test_four_mode_combinations_agree(curve, count, name):
    api = _key(curve)["api"]
    items = _batches(curve, count)[name]
    want = [_want(curve, it) for it in items]
    live, f = count - want.count(api.VERIFY_MALFORMED), want.count(api.VERIFY_REJECTED)
    if name == "all valid":
        assert want == [api.VERIFY_ACCEPTED] * count
    elif name == "every proof malformed":
        assert want == [api.VERIFY_MALFORMED] * count
    else:
        assert sorted(want) == sorted([api.VERIFY_ACCEPTED] * (count - 1) + [api.VERIFY_REJECTED if name == "a(x1) + 1" else api.VERIFY_MALFORMED]), (name, want)
    got = {}
    for pairing, challenges in COMBOS:
        v, ok, n = _run(curve, "merlin", items, pairing=pairing, challenges=challenges, seed=SEED)
        tap = _tap8(curve, count)
        _, ok0, n0 = _run(curve, "merlin", items, pairing=pairing, challenges=challenges, seed=SEED, verdicts=False)
        print(curve, count, name, pairing, challenges, "verdicts", v.tolist(), "all_accepted", ok, "n_checks", n, "without verdicts:", ok0, n0, "tap 8:", tap)
        assert v.tolist() == want, (name, pairing, challenges)
        assert ok0 == ok and n0 <= 1, (name, pairing, challenges)
        assert tap == ((0, 4 * count) if challenges == "device" else (8, 0)), (name, pairing, challenges, tap)   # 8: PM_ERR_STATE
        got[pairing, challenges] = (ok, n)
    assert len({ok for ok, _ in got.values()}) == 1 and got["host", "host"][0] == (want == [api.VERIFY_ACCEPTED] * count), (name, got)
    for pairing in ("host", "device"):
        assert got[pairing, "host"][1] == got[pairing, "device"][1], (name, pairing, got)
    assert got["host", "host"][1] <= _bound(count, f), (name, got)
    assert got["device", "host"][1] == (0 if live == 0 else 1 if f == 0 else 1 + live), (name, got)
