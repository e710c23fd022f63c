"""Writes solve_modmuldiv_cases.hpp, which is not committed: the literals of tests/native/solve_modmuldiv_selftest.cpp, computed with
Python integers (pow(D, -1, P)).  Per curve a table of modular multiply-divides, the Z in [0, P) with
cD (D+ - D-) Z = cN (A B + N+ - N-) (mod P) -- limb width, the limbs of the six operand lists and of the modulus as field elements, the
two literals, whether A and B are the same columns, whether the step sticks, and the limbs of Z.

    python tools/gen_solve_modmuldiv_cases.py > DIR/solve_modmuldiv_cases.hpp        and build the program with -I DIR
"""
import itertools
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polymath_amd import circuits as PC  # noqa: E402

R = {"BLS": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
     "BN": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001}
SECP = 2 ** 256 - 2 ** 32 - 977
P381 = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
COMPOSITE = 65521 * 65519
CMAX = 2 ** 32 - 1


def limbs_of(value, n, count=None):
    count = count or max(1, -(-value.bit_length() // n))
    assert 0 <= value < 1 << (n * count)
    return [(value >> (n * i)) & ((1 << n) - 1) for i in range(count)]


def value_of(limbs, n):
    return sum(v << (n * j) for j, v in enumerate(limbs))


def cases(r):
    g = PC.SplitMix64(0x6D756C646976)
    rnd = lambda bits: sum(g.next_u64() << (64 * i) for i in range(-(-bits // 64))) & ((1 << bits) - 1)
    out = []   # (name, n, kz, [A, B, N+, N-, D+, D-], P, literal, cN, cD, same)

    def add(name, n, kz, A, B, Np, Nm, Dp, Dm, P, literal=0, cN=1, cD=1, same=0):
        lists = [list(A), list(A) if same else list(B), list(Np), list(Nm), list(Dp), list(Dm)]
        assert all(0 <= v < r for v in sum(lists, []) + list(P)), name
        out.append((name, n, kz, lists, list(P), literal, cN, cD, same))

    # the moduli: (tag, P, n, kP); L = min(512, n (kP - 1) + 256) is the inversion's bound for the record
    moduli = (("secp256k1", SECP, 64, 4), ("BLS12-381 q", P381, 128, 4), ("2^512 - 1", 2 ** 512 - 1, 128, 4), ("3", 3, 64, 1), ("65521 * 65519", COMPOSITE, 16, 2))
    pairs = ((1, 1), (3, 2), (CMAX, CMAX))
    for tag, P, n, kP in moduli:
        Pl = limbs_of(P, n, kP)
        L = min(512, n * (kP - 1) + 256)
        kz = kP
        k = -(-max(P.bit_length(), 1) // n)      # the limbs of a value below P
        below = limbs_of((1 << 1024) - 1 - rnd(40), n, -(-1024 // n)) if -(-1024 // n) <= 32 else None      # a list has at most 32 limbs
        draw = lambda: rnd(P.bit_length() + 7) % P
        operands = [("0", [0]), ("1", [1]), ("P - 1", limbs_of(P - 1, n, k)), ("limbs that carry", [rnd(250) for _ in range(3)])]
        if below:
            operands.append(("a sum just below 2^1024", below))
        Y = draw() or 1
        while math.gcd(Y, P) != 1:      # the denominator of the cases that are not about it: invertible
            Y = draw() or 1
        # A, B over the named values; the tangent's literals on every second one
        for i, ((na, A), (nb, B)) in enumerate(itertools.product(operands, operands)):
            cN, cD = pairs[i % 3]
            add("%s: A = %s, B = %s, cN = %d, cD = %d" % (tag, na, nb, cN, cD), n, kz, A, B, limbs_of(draw(), n, k), [], limbs_of(Y, n, k), [], Pl, i & 1, cN, cD)
        # every combination of empty addend and denominator lists, under each pair of literals
        for i, (np_, nm_, d_) in enumerate(itertools.product((0, 1), (0, 1), (0, 1, 2))):
            cN, cD = pairs[i % 3]
            Dp, Dm = ([], []) if d_ == 0 else (limbs_of(Y, n, k), []) if d_ == 1 else (limbs_of(Y + 5, n, k + 1), [5])
            add("%s: lists N+ %d, N- %d, D+ %d, D- %d, cN = %d, cD = %d" % (tag, np_, nm_, len(Dp) > 0, len(Dm) > 0, cN, cD), n, kz, limbs_of(draw(), n, k), limbs_of(draw(), n, k),
                limbs_of(draw(), n, k) if np_ else [], limbs_of(draw(), n, k) if nm_ else [], Dp, Dm, Pl, i & 1, cN, cD)
        # A = B on the same columns: the tangent 3 X^2 / (2 Y), and a plain square
        for cN, cD in pairs:
            add("%s: A = B on the same columns, cN = %d, cD = %d" % (tag, cN, cD), n, kz, limbs_of(draw(), n, k), [], [], [], limbs_of(Y, n, k), [], Pl, 1, cN, cD, same=1)
        add("%s: A = B on the same columns, a square with an addend" % tag, n, kz, limbs_of(draw(), n, k), [], [7], [], [], [], Pl, 0, same=1)
        # D+ < D-, N+ < N-
        a, b = sorted((rnd(P.bit_length() + 30), rnd(P.bit_length() + 30)))
        add("%s: D+ < D-" % tag, n, kz, limbs_of(draw(), n, k), limbs_of(draw(), n, k), [3], [], limbs_of(a, n), limbs_of(b + 1, n), Pl, 1, 3, 2)
        add("%s: N+ < N-" % tag, n, kz, [2], [3], [1], limbs_of(a + 100, n), [5], [], Pl)
        # the Euclid's worst cases by name (cD = 1: the Euclid's u is D mod P)
        wide = max(k, -(-L // n))
        dens = [("D = 1", 1), ("D = P - 1", P - 1), ("D = (P + 1) / 2", (P + 1) // 2), ("D = (P - 1) / 2", (P - 1) // 2),
                ("D = 2^(L - 1), the bound's worst case of halvings", 1 << (L - 1)), ("D = 2^(bitlength(P) - 1)", 1 << (P.bit_length() - 1))]
        for name, D in dens:
            add("%s: %s" % (tag, name), n, kz, limbs_of(draw(), n, k), limbs_of(draw(), n, k), [], [], limbs_of(D, n, wide if "L - 1" in name else None), [], Pl, len(out) & 1)
        add("%s: the modulus in limbs that carry" % tag, n, kz, limbs_of(draw(), n, k), limbs_of(draw(), n, k), [], [], limbs_of(Y, n, k), [],
            [Pl[0] + (1 << n), Pl[1] - 1] + Pl[2:] if kP > 1 and Pl[1] > 0 else Pl)
        add("%s: stuck: D = 0" % tag, n, kz, [2], [3], [], [], [0], [], Pl)
        add("%s: stuck: D = P itself" % tag, n, kz, [2], [3], [], [], Pl, [], Pl, 1)
    # the composite modulus: cD D = 0 mod P though D != 0 mod P, and shared factors
    Pl = limbs_of(COMPOSITE, 16, 2)
    add("stuck: cD D = 0 mod P though D != 0 mod P (cD = 65521, D = 65519)", 16, 2, [2], [3], [], [], [65519], [], Pl, 0, 1, 65521)
    add("cD = 65522, D = 65518: invertible", 16, 2, [2], [3], [], [], [65518], [], Pl, 0, 1, 65522)
    add("stuck: cD = 65519 shares a factor with P, no denominator lists", 16, 2, [2], [3], [], [], [], [], Pl, 1, 5, 65519)
    add("cD = 65520, no denominator lists: Z = cN A B / cD", 16, 2, [2], [3], [], [], [], [], Pl, 1, 5, 65520)
    add("stuck: D = 65521 shares a factor with P", 16, 2, [2], [3], [], [], [65521], [], Pl)
    add("cN = 65521 shares a factor with P: it completes", 16, 2, [2], [3], [1], [], [7], [], Pl, 0, 65521, 1)
    # the stuck conditions, each at its boundary and one beside it
    full = (1 << 128) - 1
    S = limbs_of(SECP, 64, 4)
    Q = limbs_of(P381, 128, 4)
    add("stuck: P even", 64, 4, [5], [6], [], [], [3], [], limbs_of(SECP - 1, 64, 4))
    add("stuck: P even, literal", 64, 4, [5], [6], [], [], [3], [], limbs_of(SECP + 1, 64, 4), 1)
    add("stuck: P = 0", 64, 1, [5], [6], [], [], [3], [], [0])
    add("stuck: P = 1", 64, 1, [5], [6], [], [], [], [], [1])
    add("stuck: P = 2", 64, 1, [5], [6], [], [], [3], [], [2], 1)
    add("P = 3 is the smallest modulus", 64, 1, [5], [7], [], [], [2], [], [3])
    add("stuck: P = 2^512 exactly", 128, 4, [5], [6], [], [], [3], [], [1, 0, 0, 1 << 128])
    add("stuck: P = 2^512 + 1 by carries, literal", 128, 4, [5], [6], [], [], [3], [], [1 + (1 << 128), full, full, full], 1)
    add("P = 2^512 - 1 in limbs that carry", 128, 4, [5], [6], [], [], [7], [], [full + (1 << 128), full - 1, full, full])
    big = [0] * 7 + [1 << 128]            # 2^1024 exactly
    less = [full] * 8                     # one less
    one = [1]
    for i, tag in enumerate(("A", "B", "N+", "N-", "D+", "D-")):
        for name, v in (("stuck: %s = 2^1024 exactly" % tag, big), ("%s = 2^1024 - 1" % tag, less)):
            lists = [one, one, one, [], [3], []]
            lists[i] = v
            if tag == "D-":
                lists[4] = less if v is big else [full - 2] + [full] * 7      # D = D+ - D- stays invertible where it is not stuck
                if v is less:
                    lists[4], lists[5] = less, [full - 2] + [full] * 7
            add(name, 128, 4, *lists, Q, i & 1, 3, 2)
    add("stuck: D- = 2^1024 by carries", 128, 4, one, one, [], [], [3], [1 << 128] + [full] * 7, Q)
    add("all six lists 2^1024 - 1 or just below", 128, 4, less, [full - 1] + [full] * 7, less, [full - 7] + [full] * 7, less, [full - 12345] + [full] * 7, Q, 0, CMAX, CMAX)
    add("stuck: D+ = D-", 64, 4, [5], [6], [], [], [9, 9, 9], [9, 9, 9], S)
    add("stuck: D = 2 P in limbs that are not normalised", 64, 4, [5], [6], [], [], [2 * v for v in S], [], S)
    # Z at the edge of its kz limbs: A B = Z with D = 1
    add("stuck: Z = 2^(n kz)", 64, 2, [1 << 64], [1 << 64], [], [], [], [], S)
    add("Z = 2^(n kz) - 1", 64, 2, [1 << 64], [1 << 64], [], [1], [], [], S, 1)
    add("n = 1, kz = 16", 1, 16, [1] * 9, [1, 0, 1], [1], [], [1, 1, 0, 1], [], [1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 1])
    add("n = 86", 86, 3, limbs_of(rnd(250), 86, 3), limbs_of(rnd(255), 86, 3), limbs_of(rnd(256) % SECP, 86, 3), limbs_of(rnd(200), 86, 3), limbs_of(rnd(256) % SECP, 86, 3), [9],
        limbs_of(SECP, 86, 3), 1, 3, 2)
    add("a limb equal to r - 1", 64, 4, [r - 1, 5], [1, r - 1], [r - 1], [r - 1, r - 1], [r - 1, r - 1], [7], S)
    add("a curve with a != 0: the numerator 3 X^2 + a is N+ = a", 64, 4, limbs_of(rnd(256) % SECP, 64, 4), [], [7], [], limbs_of(rnd(256) % SECP or 1, 64, 4), [], S, 1, 3, 2, same=1)
    rows = []
    for name, n, kz, lists, P, literal, cN, cD, same in out:
        sums = [value_of(v, n) for v in lists]
        Pv = value_of(P, n)
        stuck = Pv % 2 == 0 or Pv < 3 or Pv >= 1 << 512 or any(v >= 1 << 1024 for v in sums)
        Z = 0
        if not stuck:
            N = cN * (sums[0] * sums[1] + sums[2] - sums[3]) % Pv
            D = cD * ((sums[4] - sums[5]) if lists[4] or lists[5] else 1) % Pv
            stuck = math.gcd(D, Pv) != 1
            if not stuck:
                Z = N * pow(D, -1, Pv) % Pv
                assert (Z * D - N) % Pv == 0
                stuck = Z >= 1 << (n * kz)
        named = "stuck" in name
        if stuck and not named:      # a drawn denominator may share a factor with a modulus that is not prime
            assert Pv in (3, COMPOSITE, 2 ** 512 - 1) and math.gcd(D, Pv) != 1, name
            name += " (no inverse: cD D shares a factor with P)"
        assert named <= stuck, name
        rows.append((name, n, kz, lists, P, literal, cN, cD, same, int(stuck), limbs_of(0 if stuck else Z, n, kz)))
    return rows


def words(v):
    return "{%s}" % ", ".join("0x%016xull" % ((v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF) for i in range(4))


def main():
    print("// Generated by tools/gen_solve_modmuldiv_cases.py with Python integers; do not edit.  The literals of solve_modmuldiv_selftest.cpp.")
    print("#pragma once\n#include <stdint.h>\n")
    print("// at: its first element in the pool: A, B (absent where `same`: B names A's columns), N+, N-, D+, D-, P, Z")
    print("struct ModMulDivCase { const char *name; uint32_t n, kz, k[6], kP, literal, cN, cD, same, stuck, at; };\n")
    for tag, r in R.items():
        pool, table = [], []
        for name, n, kz, lists, P, literal, cN, cD, same, stuck, Z in cases(r):
            table.append('    {"%s", %d, %d, {%s}, %d, %d, %du, %du, %d, %d, %d},' % (name, n, kz, ", ".join(str(len(v)) for v in lists), len(P), literal, cN, cD, same, stuck, len(pool)))
            pool += sum((v for i, v in enumerate(lists) if not (same and i == 1)), []) + P + Z
        print("static const ModMulDivCase MODMULDIV_%s[] = {\n%s\n};" % (tag, "\n".join(table)))
        print("static const uint64_t MODMULDIV_POOL_%s[][4] = {\n%s\n};\n" % (tag, "\n".join("    %s," % words(v) for v in pool)))


if __name__ == "__main__":
    main()
