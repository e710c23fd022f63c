"""Child process of tests/test_gpu_ntt_schedules.py::test_ntt_full_size_above_2p24_on_the_device: one domain above 2^24 through
pm_ntt_device on torch tensors, every check on the device (no host array of the domain's size exists).

  python tests/ntt_device_child.py <curve> <log_n>

A process of its own because torch brings its own HIP runtime: it has to be imported BEFORE libpolymath_hip.so is loaded, which a
pytest session that has already created its GPU context cannot do.  Prints one JSON line: {"skip": reason} when hipMemGetInfo
reports less free memory than the size needs, else {"checks": {name: bool}, "wall_s": seconds}.  (Test infrastructure; imports
oracle/ for the field constants only.)"""
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.pyref.fields import CURVES   # noqa: E402
from polymath_amd import api              # noqa: E402


def dev(vals):
    """Python integers < 2^256 -> an int64 tensor [len, 4] of their 64-bit limbs on the device, taken as they are."""
    limbs = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()
    return torch.from_numpy(limbs.view(np.int64)).to("cuda")


def dense_chunks(n, seed):
    """The dense input of the round trip, regenerated chunk by chunk (no second array of the domain's size): rows of four
    uniformly random 64-bit words (torch.randint, two 32-bit halves) with the top one cut to 61 bits -- any 253-bit value is
    canonical in both fields."""
    step = min(n, 1 << 24)
    for s in range(0, n, step):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed + s // step)
        hi = torch.randint(0, 1 << 32, (step, 4), dtype=torch.int64, device="cuda", generator=g)
        lo = torch.randint(0, 1 << 32, (step, 4), dtype=torch.int64, device="cuda", generator=g)
        v = (hi << 32) | lo
        v[:, 3] &= (1 << 61) - 1
        yield s, s + step, v


def main(curve, log_n):
    c = CURVES[curve]
    n, r = 1 << log_n, c.r
    need = (40 << 30) >> (28 - log_n)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        return {"skip": "2^%d needs %d GiB of free device memory (40 GiB at 2^28), hipMemGetInfo reports %.1f GiB" % (log_n, need >> 30, free / 2.0**30)}
    t0 = time.perf_counter()
    rnd = random.Random(1000 + log_n)
    w = pow(c.two_adic_root, 1 << (c.two_adicity - log_n), r)
    winv, ninv = pow(w, -1, r), pow(n, -1, r)
    checks = {}
    ctx = api.Context(0)          # its own context, closed below: at 2^28 the tables are ~19 GB, data + temporary 16 GB
    try:
        x = torch.empty((n, 4), dtype=torch.int64, device="cuda")

        def transform(inverse):
            # the context runs on a non-blocking stream of its own: torch's writes to x have to be complete before the call
            # (the call itself returns after the transform has finished)
            torch.cuda.synchronize()
            ctx.ntt_device(curve, x.data_ptr(), log_n, inverse)

        # constant input c -> [n c, 0, ..., 0]
        cval = rnd.randrange(1, r)
        x[:] = dev([cval])
        transform(False)
        checks["constant: output 0 is n c"] = torch.equal(x[:1], dev([n * cval % r]))
        checks["constant: all other outputs are 0"] = not bool(x[1:].any())
        # inverse of c e_0 -> c / n everywhere
        x.zero_()
        x[:1] = dev([cval])
        transform(True)
        checks["inverse of c e_0 is c / n everywhere"] = bool((x == dev([cval * ninv % r])).all())
        # 16 non-zero entries -> sum_j v_j w^(jk) at 64 positions, Python big integers
        pos = [0, 1, n // 2, n - 1]
        while len(pos) < 16:
            p = rnd.randrange(n)
            if p not in pos:
                pos.append(p)
        vals = [rnd.randrange(1, r) for _ in pos]
        ks = [0, 1, n // 2, n - 1] + [rnd.randrange(n) for _ in range(60)]
        kd = torch.tensor(ks, dtype=torch.int64, device="cuda")
        for inverse in (False, True):
            x.zero_()
            x[torch.tensor(pos, dtype=torch.int64, device="cuda")] = dev(vals)
            transform(inverse)
            root, scale = (winv, ninv) if inverse else (w, 1)
            want = [scale * sum(v * pow(root, j * k % n, r) for j, v in zip(pos, vals)) % r for k in ks]
            checks["sparse: 64 outputs, inverse=%d" % inverse] = torch.equal(x[kd], dev(want))
        # dense round trip
        seed = 77 * log_n
        for s, e, v in dense_chunks(n, seed):
            x[s:e] = v
        transform(False)
        checks["dense: forward(a) != a"] = not all(torch.equal(x[s:e], v) for s, e, v in dense_chunks(n, seed))
        transform(True)
        checks["dense: inverse(forward(a)) == a"] = all([torch.equal(x[s:e], v) for s, e, v in dense_chunks(n, seed)])
    finally:
        ctx.close()
    return {"checks": checks, "wall_s": round(time.perf_counter() - t0, 2)}


if __name__ == "__main__":
    print(json.dumps(main(sys.argv[1], int(sys.argv[2]))))
