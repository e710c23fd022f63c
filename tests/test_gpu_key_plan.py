"""GPU: resident proving keys against the pinned key plan (host/key_plan.hpp through tests/native/key_plan_selftest.cpp --print), on the
smallest keys there are: the reference's dummy circuit (n = 8) on 1 and 2 ranks and the synthetic circuit of 9 gates (n = 32) on 1, 2
and 4, every rank, both shard layouts, both curves.  What pm_pk_info, pm_pk_msm_pieces and pm_pk_msm_plan report of a key is what the
plan's row says; a base range across two resident pieces is refused on a shard and served by the whole key; and a key whose build fails
at its last point gives all of its device memory back."""
import os
import subprocess

import numpy as np
import pytest
import torch        # noqa: F401  before libpolymath_hip.so is loaded: torch brings its own HIP runtime (tests/ntt_device_child.py)

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {"pairs": 0, "vector": 1}
X_POWERS, LCS = 0, 5


@pytest.fixture(scope="module")
def plan_rows(tmp_path_factory):
    """{(m0, mw, nr, rank, count, layout): the fields of the K row} from the self-test's print mode"""
    exe = str(tmp_path_factory.mktemp("key_plan") / "key_plan_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "key_plan_selftest.cpp")])
    rows = {}
    for line in subprocess.run([exe, "--print"], capture_output=True, text=True, check=True).stdout.splitlines():
        cells = line.split(" : ")
        head = cells[0].split()
        if head[0] != "K" or head[1] != "32" or head[8] != "0":
            continue
        rows[tuple(int(v) for v in head[2:8])] = cells[1:]
    return rows


def _circuits(curve, pm):
    from polymath_amd import circuits as PC
    from polymath_amd.polymath import Field, LimbCircuit, _csr
    c, f, g = CURVES[curve], Field(curve), PC.SplitMix64(0x6B70)

    def limb_circuit(r1cs, inst, wit):
        return LimbCircuit(f, r1cs.m0, r1cs.mw, r1cs.nr, (_csr(f, r1cs.a), _csr(f, r1cs.b), _csr(f, r1cs.c)), f.fr_limbs(inst), f.fr_limbs(wit))
    dummy = limb_circuit(*pm._synthesize(PC.DummyCircuit(g.fr(c.r), g.fr(c.r))))
    nine = limb_circuit(*PC.synthetic_r1cs(c.r, 9))
    return g, [(dummy, 8, (1, 2)), (nine, 32, (1, 2, 4))]


@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_resident_keys_are_the_pinned_plan(gpu_ctx, plan_rows, curve):
    from polymath_amd.polymath import Polymath
    c = CURVES[curve]
    pm = Polymath(curve, "merlin", ctx=gpu_ctx)
    g, circuits = _circuits(curve, pm)
    for lc, n, ranks in circuits:
        x, z = g.fr(c.r), g.fr(c.r)
        for layout in ("pairs", "vector"):
            for N in ranks:
                for rank in range(N):
                    row = plan_rows[(lc.m0, lc.mw, lc.nr, rank, N, LAYOUTS[layout])]
                    assert row[0] == "0", (n, layout, N, rank)
                    pk = pm.setup(lc, x, z, rank, N, layout)
                    plan_n, _, plan_sigma = (int(v) for v in row[1].split())
                    assert (pk.n, pk.m0, pk.sigma) == (plan_n, lc.m0, plan_sigma) and pk.n == n
                    assert pk.base_lens == [int(v) for v in row[2].split()]
                    res_cnt = [int(v) for v in row[7].split()]
                    for which in range(3):
                        cell = row[10 + which].split()
                        assert cell[0] == "acd"[which]
                        assert pk.msm_pieces(which) == [tuple(int(v) for v in pc.split("+")) for pc in cell[1:]], (n, layout, N, rank, which)
                        assert pk.msm_plan(which)[0] == res_cnt[which] == sum(cnt for _, cnt in pk.msm_pieces(which))
                    pk.free()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_a_range_across_two_pieces_is_refused_on_a_shard(gpu_ctx, curve):
    """n = 32 on 2 ranks: rank 0 holds x_powers [0, 8) and [16, 24) as pieces of [a]_1, [0, 9) and [16, 25) as pieces of [c]_1 (vector
    layout), or [0, 17) as its slice of [a]_1 (pair layout).  [6, 18) and [15, 19) lie in no single piece."""
    from polymath_amd import api
    from polymath_amd.polymath import Polymath
    c = CURVES[curve]
    pm = Polymath(curve, "merlin", ctx=gpu_ctx)
    g, circuits = _circuits(curve, pm)
    lc = circuits[1][0]
    x, z = g.fr(c.r), g.fr(c.r)
    whole = pm.setup(lc, x, z)
    assert whole.n == 32
    xp = whole.export_bases(X_POWERS)
    assert xp.shape[0] == 33 and np.array_equal(whole.export_bases(X_POWERS, 6, 12), xp[6:18])
    for layout, inside, across in (("vector", [(0, 9), (16, 9), (17, 7)], (6, 12)), ("pairs", [(0, 17), (3, 10)], (15, 4))):
        shard = pm.setup(lc, x, z, 0, 2, layout)
        for off, cnt in inside:
            assert np.array_equal(shard.export_bases(X_POWERS, off, cnt), xp[off:off + cnt]), (layout, off, cnt)
        with pytest.raises(api.PolymathError) as ex:
            shard.export_bases(X_POWERS, *across)
        assert ex.value.status == 1, layout                      # PM_ERR_INVALID_ARG: not resident on this shard
        with pytest.raises(api.PolymathError) as ex:
            shard.export_bases_compressed(X_POWERS, *across)
        assert ex.value.status == 1, layout
        shard.free()
    whole.free()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_a_key_refused_at_its_last_point_gives_its_memory_back(gpu_ctx, curve):
    """The byte loader reads its verdicts after matrices, segment lists and all resident points are on the device: a refused last point
    of the last vector is the latest a build fails without a HIP error.  Free device memory is where it was, and the next key builds."""
    from polymath_amd import api
    from polymath_amd.polymath import Polymath
    c = CURVES[curve]
    pm = Polymath(curve, "merlin", ctx=gpu_ctx)
    g, circuits = _circuits(curve, pm)
    lc = circuits[1][0]
    x, z = g.fr(c.r), g.fr(c.r)
    pk = pm.setup(lc, x, z)
    data = pm.pk_serialize(pk, lc, pm.make_vk(pk, x, z))
    lcs = pk.export_bases(LCS)
    pk.free()
    nb = 48 if curve == "bls12_381" else 32
    ge_p = bytes([c.p.to_bytes(48, "big")[0] | 0x80]) + c.p.to_bytes(48, "big")[1:] if curve == "bls12_381" else c.p.to_bytes(32, "little")
    corrupt = data[:-nb] + ge_p                                # the key's last record: uj_wj_lcs[Lz - 1], x = p

    def refused(rank, count, layout):
        with pytest.raises(api.PolymathError) as ex:
            pm.pk_load_bytes(corrupt, True, rank, count, layout)
        assert ex.value.status == 1
        assert "pm_pk_load_bytes: uj_wj_lcs_by_y_alpha_g1[%d]: G1: coordinate >= p" % (lcs.shape[0] - 1) in str(ex.value), str(ex.value)
    # the whole key, and the ranks of 2 that hold the last lcs point: rank 0's slice of [c]_1, rank 1's part of z_tail (the vector layout
    # has the two segment lists on the device as well)
    for rank, count, layout in ((0, 1, "pairs"), (0, 2, "pairs"), (1, 2, "vector")):
        refused(rank, count, layout)                           # once before measuring: the context's own workspaces settle
        free_before = torch.cuda.mem_get_info()[0]
        refused(rank, count, layout)
        assert torch.cuda.mem_get_info()[0] == free_before, (rank, count, layout)
    again, _ = pm.pk_load_bytes(data)
    assert np.array_equal(again.export_bases(LCS), lcs)
    again.free()
