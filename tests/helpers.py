"""Shared helpers for the test-suite (test infrastructure; may import oracle/)."""
import json
import os

import numpy as np

from oracle import cpp_oracle as CO
from oracle.pyref import protocol as PR
from oracle.pyref.fields import CURVES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I = lambda s: int(s, 16)
PT = lambda p: None if p is None else (int(p[0], 16), int(p[1], 16))
BASE_NAMES = CO.OraclePk.BASE_NAMES  # pm_base_vec order


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def r1cs_from_json(j):
    row = lambda rw: [(int(v, 16), c) for v, c in rw]
    return PR.R1CS(j["m0"], j["mw"], [row(r) for r in j["a"]], [row(r) for r in j["b"]], [row(r) for r in j["c"]])


def rand_fr_limbs(curve, count, seed):
    """count uniformly random Fr elements as Montgomery limbs [count,4] (numpy RNG; rejection)."""
    r = CURVES[curve].r
    rng = np.random.default_rng(seed)
    top_mask = (1 << (r.bit_length() - 192)) - 1
    out = rng.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
    out[:, 3] &= np.uint64(top_mask)
    # reject >= r (compare top limb only is not exact; fix rare rows exactly)
    r_limbs = [(r >> (64 * k)) & ((1 << 64) - 1) for k in range(4)]
    bad = out[:, 3] >= np.uint64(r_limbs[3])
    for i in np.nonzero(bad)[0]:
        v = sum(int(out[i, k]) << (64 * k) for k in range(4))
        while v >= r:
            v >>= 1
        for k in range(4):
            out[i, k] = (v >> (64 * k)) & ((1 << 64) - 1)
    return out


def pm_csrs(curve, r1cs):
    """Three polymath_amd.api.CsrArrays (A, B, C) for an R1CS given with integer coefficients."""
    from polymath_amd import api
    out = []
    for rows in (r1cs.a, r1cs.b, r1cs.c):
        rowptr, cols, vals = [0], [], []
        for row in rows:
            for v, j in row:
                cols.append(j)
                vals.append(v)
            rowptr.append(len(cols))
        out.append(api.CsrArrays(rowptr, cols, CO.fr_to_mont_limbs(curve, vals) if vals else []))
    return out


TABLES_OPT = {"1": "auto", "0": "off", "wide": "wide"}     # the parametrisations' historical names (PM_TABLES values)


# ------------------------------------------------------------------ degenerate MSM inputs
# Shared by test_msm_degenerate_inputs.py (CPU: the two references agree on every family) and test_gpu_msm_degenerate.py (the
# kernels against both).  Every base is a KNOWN multiple k_i G -- k = 0 the point at infinity, k < 0 the negated point -- so every
# MSM has the closed form (sum s_i k_i mod r) G next to the oracle's Pippenger.  Scalars are Python integers: a list of len(ks)
# values, or a dict {index: value} (all other scalars zero) for the probes that place a handful of contributions.
def fr_mont_limbs(curve, vals):
    """Python integers -> Montgomery limbs [len, 4] (oracle.fr_to_mont_limbs without the per-limb Python loop)."""
    c = CURVES[curve]
    buf = b"".join(c.fr_to_mont(v % c.r).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def _negate_fq_limbs(curve, y):
    """p - y on [m, nq] little-endian 64-bit limbs (y != 0 mod p): the Montgomery form of -y is p minus the Montgomery form of y."""
    c = CURVES[curve]
    out = np.empty_like(y)
    borrow = np.zeros(len(y), dtype=np.uint64)
    for k in range(c.fq_limbs64):
        pk = np.uint64((c.p >> (64 * k)) & ((1 << 64) - 1))
        t = pk - y[:, k]                                   # wraps where y_k > p_k
        out[:, k] = t - borrow
        borrow = ((y[:, k] > pk) | (t < borrow)).astype(np.uint64)
    assert not borrow.any()
    return out


def signed_multiples(curve, ks):
    """The bases k_i G as Montgomery limbs [len, 2 nq]: all-zero rows for k = 0, (x, p - y) for k < 0.  Magnitudes come from
    oracle.g1_multiples (the running sum G, 2G, ...), or from oracle.g1_mul where only a few distinct ones occur."""
    nq = CURVES[curve].fq_limbs64
    ks = np.asarray(ks, dtype=np.int64)
    mags = np.abs(ks)
    out = np.zeros((len(ks), 2 * nq), dtype=np.uint64)
    uniq = np.unique(mags[mags > 0])
    if len(uniq) > 64:
        table = CO.g1_multiples(curve, int(uniq[uniq <= 1 << 18][-1]))
        small = (mags > 0) & (mags <= len(table))
        out[small] = table[mags[small] - 1]
        uniq = uniq[uniq > len(table)]
    g = CO.g1_multiples(curve, 1)[0]
    for m in uniq:
        pt, inf = CO.g1_mul(curve, g, fr_mont_limbs(curve, [int(m)])[0])
        assert inf == 0
        out[mags == m] = pt
    neg = ks < 0
    out[neg, nq:] = _negate_fq_limbs(curve, out[neg, nq:])
    return out


def scalar_limbs(curve, n, scalars):
    """A scalar vector (list, or dict of the non-zero entries) as Montgomery limbs [n, 4]."""
    if isinstance(scalars, dict):
        out = np.zeros((n, 4), dtype=np.uint64)
        idx = sorted(scalars)
        out[idx] = fr_mont_limbs(curve, [scalars[i] for i in idx])
        return out
    assert len(scalars) == n
    return fr_mont_limbs(curve, scalars)


def msm_closed_form(curve, ks, scalars):
    """(sum s_i k_i mod r) G by one scalar multiplication (oracle.g1_mul) -> (xy, inf, the sum); infinity exactly when the sum is 0."""
    r = CURVES[curve].r
    items = scalars.items() if isinstance(scalars, dict) else enumerate(scalars)
    total = sum(int(ks[i]) * s for i, s in items) % r
    out, inf = CO.g1_mul(curve, CO.g1_multiples(curve, 1)[0], fr_mont_limbs(curve, [total])[0])
    assert inf == (1 if total == 0 else 0)
    return (np.zeros_like(out) if inf else out), inf, total


_TWO_REFERENCES = {}


def msm_two_references(curve, hb, ks, scalars, key=None, nthreads=16):
    """The two independent expectations of one MSM, asserted equal: the oracle's Pippenger (complete additions; over the non-zero
    scalars only where `scalars` is a dict -- the zero ones contribute nothing) and the closed form -> (xy, inf).  key: remembers
    the answer for the pipelines that run the same input."""
    if key is not None and key in _TWO_REFERENCES:
        return _TWO_REFERENCES[key]
    if isinstance(scalars, dict):
        idx = sorted(scalars)
        ref, rinf = CO.msm(curve, hb[idx], fr_mont_limbs(curve, [scalars[i] for i in idx]), 1)
    else:
        ref, rinf = CO.msm(curve, hb, fr_mont_limbs(curve, scalars), nthreads)
    want, winf, _ = msm_closed_form(curve, ks, scalars)
    if rinf:
        ref = np.zeros_like(ref)
    assert rinf == winf and np.array_equal(ref, want), "oracle.msm and the closed form disagree"
    if key is not None:
        _TWO_REFERENCES[key] = (want, winf)
    return want, winf


def per_window_bits(n, scalar_bits):
    """Window width of the per-window pipeline for n pairs (mirror of msm_plan.h: per_window_bits -- used only to AIM the probes)."""
    best, bc = None, 4
    for c in range(4, 17):
        cost = ((scalar_bits + c) // c) * (n + 6 * (1 << (c - 1)))
        if best is None or cost < best:
            best, bc = cost, c
    return bc


PIPELINE_NAMES = ["windows", "tables16", "tables12-small", "tables-auto"]


def msm_pipeline(curve, name):
    """The bucket pipelines every family runs on: pairs, context options, precompute() or not, and -- where the plan is known --
    the window width c (2^(c-1) buckets per set) and the bit offsets of the c-bit windows."""
    bits = CURVES[curve].r.bit_length()
    c = per_window_bits(1 << 17, bits)
    return {
        # per-window Pippenger (no tables): LDS-histogram sort, accumulate<false>, k_bucket_reduce + k_sum_parts per window, host_horner
        "windows": dict(n=1 << 17, options={}, tables=False, c=c, offs=[c * w for w in range((bits + c) // c)]),
        # window tables, 16 windows of 16 bits, 2^15 buckets: three-level sort, accumulate<true>, the two-level reduction
        "tables16": dict(n=1 << 17, options={"table_window_bits": 16}, tables=True, c=16, offs=[16 * w for w in range(16)]),
        # window tables with 2^11 buckets (22 windows, the first 14 of 12 bits): one sort region, the single-level reduction
        "tables12-small": dict(n=1 << 11, options={"table_window_bits": 12}, tables=True, c=12, offs=[12 * w for w in range(14)]),
        # window tables, the plan the cost model picks (its layout is not mirrored here: aligned inputs use window 0)
        "tables-auto": dict(n=1 << 17, options={}, tables=True, c=None, offs=[0]),
    }[name]


def _rng(*key):
    import random
    return random.Random(repr(key))


def _pairs_layout(n, arrangement):
    """ks for n / 2 opposite pairs +-(j + 1) G and the pair index of every entry: interleaved, or +P in the first half, -P in the second."""
    m = n // 2
    j = np.arange(m, dtype=np.int64)
    if arrangement == "interleaved":
        ks = np.empty(n, dtype=np.int64)
        ks[0::2], ks[1::2] = j + 1, -(j + 1)
        return ks, np.repeat(j, 2)
    assert arrangement == "halves"
    return np.concatenate([j + 1, -(j + 1)]), np.concatenate([j, j])


def family_a(curve, n, arrangement, variant, shift=0, digit_bits=10):
    """A. Opposite pairs P_j, -P_j with EQUAL scalars: every bucket sum is O, the result is O, every scalar is non-zero.
    variant: "random" (many buckets), "repeated" (two values: a hot bucket per window for each fold tier -- 7/8 and 1/8 of the
    pairs), "aligned" (a digit of digit_bits bits at bit `shift`: the pairs sit in one window only)."""
    r = CURVES[curve].r
    rng = _rng("A", curve, n, arrangement, variant)
    ks, pair = _pairs_layout(n, arrangement)
    m = n // 2
    if variant == "random":
        sp = [rng.randrange(1, r) for _ in range(m)]
    elif variant == "repeated":
        v1, v2 = rng.randrange(1, r), rng.randrange(1, r)
        sp = [v2 if j % 8 == 3 else v1 for j in range(m)]
    else:
        assert variant == "aligned"
        sp = [rng.randrange(1, 1 << digit_bits) << shift for _ in range(m)]
    return ks, [sp[j] for j in pair]


def family_b(curve, n, variant):
    """B. Family A (interleaved) and ~n/16 (at most 384) further entries, then one fixed shuffle of the whole vector (the order inside
    a bucket is the sort's business: the shuffle and the number of buckets make every order occur).  A third of the extras is a
    THIRD copy +-P_j with its pair's scalar -- (P, -P, P), (P, P, -P), (-P, P, -P) in one bucket --, a third are duplicates
    (P_q, s), (P_q, s) with a fresh scalar (doubling), the rest fresh pairs, some at infinity.  With "repeated" the extras carry
    the hot value too, so the hot bucket's sum passes through O and goes on.  The result is not O."""
    r = CURVES[curve].r
    rng = _rng("B", curve, n, variant)
    extras = min(384, n // 16) // 6 * 6
    n0 = n - extras
    ks0, sc0 = family_a(curve, n0, "interleaved", variant)
    m = n0 // 2
    ks, sc = [int(k) for k in ks0], list(sc0)
    for e in range(extras // 3):                       # third copies
        j = rng.randrange(m)
        ks.append((j + 1) if e % 2 == 0 else -(j + 1))
        sc.append(sc0[2 * j])
    for e in range(extras // 6):                       # duplicates, two entries each
        q, s = rng.randrange(1, m + 1), (sc0[0] if variant == "repeated" and e % 2 else rng.randrange(1, r))
        ks += [q, q]
        sc += [s, s]
    for e in range(extras // 3):                       # fresh pairs
        ks.append(0 if e % 16 == 5 else rng.randrange(1, m + 1) * (1 if e % 3 else -1))
        sc.append(sc0[0] if variant == "repeated" and e % 4 == 0 else rng.randrange(1, r))
    order = list(range(n))
    rng.shuffle(order)
    return np.array([ks[i] for i in order], dtype=np.int64), [sc[i] for i in order]


def family_c(curve, n, arrangement):
    """C. The SAME base twice with scalars s and r - s: the digits differ, no bucket cancels, the total does -- in the last
    additions of the reduction or on the host."""
    r = CURVES[curve].r
    rng = _rng("C", curve, n, arrangement)
    ks, pair = _pairs_layout(n, arrangement)
    sp = [rng.randrange(1, r) for _ in range(n // 2)]
    return np.abs(ks), [sp[j] if k > 0 else r - sp[j] for j, k in zip(pair, ks)]


def family_d(curve, n, c, offs):
    """D. Two-contribution probes on one base vector: -> (ks, probes, piece_probes), probes = [(label, {index: scalar})].
    Bucket b of a window at bit offset `off` weighs b + 1, so the scalar d << off on a base puts it into bucket d - 1 (d <= 2^(c-1)).
      meet:   +G in bucket 2t - 1 and two -G (or one -2G) in bucket t - 1: X = 2t 2^off G and -X, first added to each other where the
              reduction brings the two buckets together; t = 1, 2, 4, ... NB1 / 2 moves that node from one lane through the LDS
              tree to different workgroups and the final sum.  With +G / +2G in the second slot: X + X at the same node.
      cross:  the two contributions in neighbouring windows (bases +-2^(c+1) G one window down): host_horner without tables, two
              buckets of the shared set with; and 2^c G against -+G one window up: without tables again host_horner, with tables the
              SAME table point twice in one bucket (k_accumulate).
      lane:   G in bucket b and +-G in bucket b - 1, b odd (one reduction lane owns both): the lane's running sum meets an equal /
              opposite bucket.
      pieces: +G in the first half of the vector and +-G in the second with one random scalar: the sum over pieces in msm_run,
              when msm_max_piece_log splits the vector there."""
    r = CURVES[curve].r
    rng = _rng("D", curve, n, c)
    nb1 = 1 << (c - 1)
    ks = np.array([(i % 97) + 1 for i in range(n)], dtype=np.int64)       # zero scalars everywhere else
    names = ["G", "nG1", "nG2", "n2G", "G1", "G2", "2G", "Gc", "nGc1", "Gc1"]
    vals = [1, -1, -1, -2, 1, 1, 2, 1 << c, -(1 << (c + 1)), 1 << (c + 1)]
    at = {nm: (n // 2) * (7 * i + 3) // (7 * len(names)) for i, nm in enumerate(names)}      # spread over the first half
    at.update(hG=n // 2 + n // 5, hnG=n - 3)
    for nm, v in zip(names + ["hG", "hnG"], vals + [1, -1]):
        ks[at[nm]] = v
    mid = offs[min(5, len(offs) - 1)]
    probes = []
    t = 1
    while t <= nb1 // 2:
        for off in (offs[0], mid):
            probes.append(("meet-cancel-2x-G t=%d off=%d" % (t, off), {at["G"]: 2 * t << off, at["nG1"]: t << off, at["nG2"]: t << off}))
            probes.append(("meet-double-2x+G t=%d off=%d" % (t, off), {at["G"]: 2 * t << off, at["G1"]: t << off, at["G2"]: t << off}))
        probes.append(("meet-cancel-2G t=%d off=%d" % (t, mid), {at["G"]: 2 * t << mid, at["n2G"]: t << mid}))
        probes.append(("meet-double+2G t=%d off=%d" % (t, mid), {at["G"]: 2 * t << mid, at["2G"]: t << mid}))
        t <<= 1
    w = min(5, len(offs) - 1)
    lo, hi = offs[w - 1], offs[w]
    assert hi - lo == c
    for t in sorted({1, 3, 64, nb1 // 2 - 1, nb1 // 2}):
        probes.append(("cross-cancel t=%d" % t, {at["G"]: 2 * t << hi, at["nGc1"]: t << lo}))
        probes.append(("cross-double t=%d" % t, {at["G"]: 2 * t << hi, at["Gc1"]: t << lo}))
        probes.append(("cross-same-point-cancel d=%d" % t, {at["Gc"]: t << lo, at["nG1"]: t << hi}))
        probes.append(("cross-same-point-double d=%d" % t, {at["Gc"]: t << lo, at["G1"]: t << hi}))
    for b in sorted({1, 3, 7, nb1 // 2 + 1, nb1 - 1}):
        for off in (offs[0], mid):
            probes.append(("lane-opposite b=%d off=%d" % (b, off), {at["G"]: (b + 1) << off, at["nG1"]: b << off}))
            probes.append(("lane-equal b=%d off=%d" % (b, off), {at["G"]: (b + 1) << off, at["G1"]: b << off}))
    s1, s2 = rng.randrange(1, r), rng.randrange(1, r)
    pieces = [("pieces-cancel", {at["G"]: s1, at["hnG"]: s1}), ("pieces-double", {at["G"]: s2, at["hG"]: s2}),
              ("pieces-cancel-then-more", {at["G"]: s1, at["hnG"]: s1, at["2G"]: s2, at["hG"]: 5})]
    return ks, probes, pieces


def family_e(curve, n, max_digit, vectors):
    """E. Bases +-G at random, scalars 1 ... max_digit (one digit, window 0): every bucket holds a few +G and -G, its sum is a small
    multiple of G of either sign or O, the running sums walk through 0.  `vectors` seeded scalar vectors on the one base vector."""
    rng = _rng("E", curve, n, max_digit)
    ks = np.array([1 if rng.getrandbits(1) else -1 for _ in range(n)], dtype=np.int64)
    return ks, [[rng.randrange(1, max_digit + 1) for _ in range(n)] for _ in range(vectors)]


def family_f(curve, n):
    """F. The multiples 1 ... n in random order with ~1 % points at infinity, ~1 % exact duplicates and ~1 % negated duplicates of
    other entries; random scalars with a few 0, 1 and r - 1."""
    r = CURVES[curve].r
    rng = _rng("F", curve, n)
    ks = list(range(1, n + 1))
    rng.shuffle(ks)
    special = rng.sample(range(n), 3 * max(n // 100, 4))
    third = len(special) // 3
    keep = sorted(set(range(n)) - set(special))
    for i in special[:third]:
        ks[i] = 0
    for i in special[third:2 * third]:
        ks[i] = ks[rng.choice(keep)]
    for i in special[2 * third:]:
        ks[i] = -ks[rng.choice(keep)]
    sc = [rng.randrange(1, r) for _ in range(n)]
    for i, v in zip(rng.sample(range(n), 6), (0, 0, 1, 1, r - 1, r - 1)):
        sc[i] = v
    return np.array(ks, dtype=np.int64), sc


# G. tiny vectors for pm_g1_sum and the host-stride pm_msm_g1: (label, ks); P = 5 G, Q = 11 G
FAMILY_G = [("P,-P", [5, -5]), ("P,P", [5, 5]), ("O,P,-P,O", [0, 5, -5, 0]), ("P,-P,Q", [5, -5, 11]), ("P,P,-P,-P", [5, 5, -5, -5]),
            ("P,Q,-P,-Q,P", [5, 11, -5, -11, 5])]


def patch_preimages(patch_text):
    """A unified diff -> {path: [(start, count, lines), ...]}: per hunk, the line range of the ORIGINAL file its header names
    and the lines it expects there (context and removed lines, in order).  A file the patch creates has one hunk (0, 0, [])."""
    out, path, hunk = {}, None, None
    for line in patch_text.split("\n"):
        if line.startswith("diff --git "):
            path, hunk = line.split(" b/", 1)[1], None
            out[path] = []
        elif line.startswith("@@ "):
            start, _, count = line.split()[1][1:].partition(",")
            hunk = (int(start), int(count or 1), [])
            out[path].append(hunk)
        elif hunk is not None and line[:1] in (" ", "-", ""):
            if len(hunk[2]) < hunk[1]:
                hunk[2].append(line[1:])
    return out
