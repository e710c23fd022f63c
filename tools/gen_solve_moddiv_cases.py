"""Writes solve_moddiv_cases.hpp, which is not committed: the literals of tests/native/solve_moddiv_selftest.cpp, computed with Python
integers (pow(D, -1, P)).  Per curve a table of modular divisions Z = (N+ - N-) / (D+ - D-) mod P -- limb width, the limbs of the four
operand lists and of the modulus as field elements, whether the step sticks, and the limbs of Z.

    python tools/gen_solve_moddiv_cases.py > DIR/solve_moddiv_cases.hpp        and build the program with -I DIR
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polymath_amd import circuits as PC  # noqa: E402

R = {"BLS": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
     "BN": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001}
SECP = 2 ** 256 - 2 ** 32 - 977
P381 = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
COMPOSITE = 15 * (2 ** 89 - 1)


def limbs_of(value, n, count):
    assert 0 <= value < 1 << (n * count)
    return [(value >> (n * i)) & ((1 << n) - 1) for i in range(count)]


def value_of(limbs, n):
    return sum(v << (n * j) for j, v in enumerate(limbs))


def cases(r):
    g = PC.SplitMix64(0x6D6F64646976)
    rnd = lambda bits: sum(g.next_u64() << (64 * i) for i in range(-(-bits // 64))) & ((1 << bits) - 1)
    out = []   # (name, n, kz, N+, N-, D+, D-, P, literal)

    def add(name, n, kz, Np, Nm, Dp, Dm, P, literal=0):
        assert all(0 <= v < r for v in Np + Nm + Dp + Dm + P), name
        out.append((name, n, kz, list(Np), list(Nm), list(Dp), list(Dm), list(P), literal))

    # the moduli: (tag, P, n, kP); L = min(512, n (kP - 1) + 256) is the inversion's bound for the record
    moduli = (("secp256k1", SECP, 64, 4), ("BLS12-381 q", P381, 128, 4), ("2^512 - 1", 2 ** 512 - 1, 128, 4), ("3", 3, 64, 1), ("15 (2^89 - 1)", COMPOSITE, 32, 3))
    for tag, P, n, kP in moduli:
        Pl = limbs_of(P, n, kP)
        L = min(512, n * (kP - 1) + 256)
        kz = kP
        k = -(-max(P.bit_length(), 1) // n)     # the limbs of a value below P
        wide = max(k, -(-L // n))                # the limbs of 2^(L - 1)
        N = rnd(P.bit_length() + 7) % P
        dens = [("D = 1", 1), ("D = P - 1", P - 1), ("D = (P + 1) / 2", (P + 1) // 2), ("D = (P - 1) / 2", (P - 1) // 2),
                ("D = 2^(L - 1), the bound's worst case of halvings", 1 << (L - 1)), ("D = 2^(bitlength(P) - 1)", 1 << (P.bit_length() - 1)),
                ("D = 0", 0), ("D = P itself", P), ("D random", rnd(P.bit_length() + 60))]
        for name, D in dens:
            kD = max(1, -(-max(D.bit_length(), 1) // n))
            add("%s: %s" % (tag, name), n, kz, limbs_of(N, n, k), [], limbs_of(D, n, max(kD, wide if "L - 1" in name else kD)), [], Pl, len(out) & 1)
        # N = 1 (a plain inverse: no numerator lists), D+ < D-, N+ < N-, limbs that are not normalised and carry
        D = rnd(P.bit_length() + 7) % P
        add("%s: N = 1" % tag, n, kz, [], [], limbs_of(D or 1, n, k), [], Pl)
        a, b = sorted((rnd(P.bit_length() + 30), rnd(P.bit_length() + 30)))
        add("%s: D+ < D-" % tag, n, kz, limbs_of(N, n, k), [], limbs_of(a, n, -(-a.bit_length() // n) or 1), limbs_of(b + 1, n, -(-(b + 1).bit_length() // n)), Pl, 1)
        add("%s: N+ < N-, N+ empty" % tag, n, kz, [], limbs_of(N or 1, n, k), limbs_of(D or 1, n, k), [], Pl)
        add("%s: limbs of 250 bits that carry, in all four lists" % tag, n, kz, [rnd(250) for _ in range(3)], [rnd(250) for _ in range(2)], [rnd(250) for _ in range(4)],
            [rnd(250) for _ in range(3)], Pl, 1)
        add("%s: the modulus in limbs that carry" % tag, n, kz, limbs_of(N, n, k), [], limbs_of(D or 1, n, k), [],
            [Pl[0] + (1 << n), Pl[1] - 1] + Pl[2:] if kP > 1 and Pl[1] > 0 else Pl)
    # a denominator that shares a factor with the composite modulus: no inverse, though D != 0 mod P
    Pl = limbs_of(COMPOSITE, 32, 3)
    for factor in (3, 5, 15, 2 ** 89 - 1, 21 * (2 ** 89 - 1)):
        add("15 (2^89 - 1): D = %d shares a factor" % factor, 32, 3, [7], [], limbs_of(factor, 32, 4), [], Pl)
    add("15 (2^89 - 1): D = 7 is invertible though P is composite", 32, 3, [7], [], [7 + 3], [3], Pl)
    # the stuck conditions, each at its boundary and one beside it
    full = (1 << 128) - 1
    S = limbs_of(SECP, 64, 4)
    add("stuck: P even", 64, 4, [5], [], [3], [], limbs_of(SECP - 1, 64, 4))
    add("stuck: P even, literal", 64, 4, [5], [], [3], [], limbs_of(SECP + 1, 64, 4), 1)
    add("stuck: P = 0", 64, 1, [5], [], [3], [], [0])
    add("stuck: P = 1", 64, 1, [5], [], [3], [], [1])
    add("stuck: P = 2", 64, 1, [5], [], [3], [], [2], 1)
    add("P = 3 is the smallest modulus", 64, 1, [5], [], [2], [], [3])
    add("stuck: P = 2^512 exactly", 128, 4, [5], [], [3], [], [1, 0, 0, 1 << 128])
    add("stuck: P = 2^512 + 1 by carries, literal", 128, 4, [5], [], [3], [], [1 + (1 << 128), full, full, full], 1)
    add("P = 2^512 - 1 in limbs that carry", 128, 4, [5], [], [3], [], [full + (1 << 128), full - 1, full, full])
    big = [0] * 7 + [1 << 128]
    most = [full] * 8
    add("stuck: N+ = 2^1024", 128, 4, big, [], [3], [], limbs_of(P381, 128, 4))
    add("stuck: N- = 2^1024", 128, 4, [1], big, [3], [], limbs_of(P381, 128, 4))
    add("stuck: D+ = 2^1024", 128, 4, [1], [], big, [], limbs_of(P381, 128, 4), 1)
    add("stuck: D- = 2^1024 by carries", 128, 4, [1], [], [3], [1 << 128] + [full] * 7, limbs_of(P381, 128, 4))
    add("all four lists 2^1024 - 1 or just below", 128, 4, most, [full - 1] + [full] * 7, most, [full - 12345] + [full] * 7, limbs_of(P381, 128, 4))
    add("stuck: D+ = D-", 64, 4, [5], [], [9, 9, 9], [9, 9, 9], S)
    add("stuck: D = 2 P in limbs that are not normalised", 64, 4, [5], [], [2 * v for v in S], [], S)
    Z = 1 << 128
    D = pow(Z, -1, SECP)
    add("stuck: Z = 2^(n kz)", 64, 2, [], [], limbs_of(D, 64, 4), [], S)
    D = pow(Z - 1, -1, SECP)
    add("Z = 2^(n kz) - 1", 64, 2, [], [], limbs_of(D, 64, 4), [], S, 1)
    add("n = 1, kz = 16", 1, 16, [1] * 9, [], [1, 1, 0, 1], [], [1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 1])
    add("n = 86", 86, 3, limbs_of(rnd(250), 86, 3), limbs_of(rnd(255), 86, 3), limbs_of(rnd(256) % SECP, 86, 3), limbs_of(rnd(200), 86, 3), limbs_of(SECP, 86, 3), 1)
    add("a limb equal to r - 1", 64, 4, [r - 1, 5], [1, r - 1], [r - 1, r - 1], [7], S)
    rows = []
    for name, n, kz, Np, Nm, Dp, Dm, P, literal in out:
        sums = [value_of(v, n) for v in (Np, Nm, Dp, Dm)]
        Pv = value_of(P, n)
        stuck = Pv % 2 == 0 or Pv < 3 or Pv >= 1 << 512 or any(v >= 1 << 1024 for v in sums)
        Z = 0
        if not stuck:
            N = (sums[0] - sums[1]) % Pv if Np or Nm else 1
            D = (sums[2] - sums[3]) % Pv
            stuck = math.gcd(D, Pv) != 1
            if not stuck:
                Z = N * pow(D, -1, Pv) % Pv
                assert Z * D % Pv == N % Pv
                stuck = Z >= 1 << (n * kz)
        named = "stuck" in name or "shares" in name or "D = 0" in name or "D = P itself" in name
        if stuck and not named:      # a drawn denominator may share a factor with a modulus that is not prime
            assert Pv in (3, COMPOSITE, 2 ** 512 - 1) and math.gcd((sums[2] - sums[3]) % Pv, Pv) != 1, name
            name += " (no inverse: it shares a factor with P)"
        assert named <= stuck, name
        rows.append((name, n, kz, Np, Nm, Dp, Dm, P, literal, int(stuck), limbs_of(0 if stuck else Z, n, kz)))
    return rows


def words(v):
    return "{%s}" % ", ".join("0x%016xull" % ((v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF) for i in range(4))


def main():
    print("// Generated by tools/gen_solve_moddiv_cases.py with Python integers; do not edit.  The literals of solve_moddiv_selftest.cpp.")
    print("#pragma once\n#include <stdint.h>\n")
    print("struct ModdivCase { const char *name; uint32_t n, kz, k[4], kP, literal, stuck, at; };   // at: its first element in the pool: N+, N-, D+, D-, P, Z\n")
    for tag, r in R.items():
        pool, table = [], []
        for name, n, kz, Np, Nm, Dp, Dm, P, literal, stuck, Z in cases(r):
            table.append('    {"%s", %d, %d, {%d, %d, %d, %d}, %d, %d, %d, %d},' % (name, n, kz, len(Np), len(Nm), len(Dp), len(Dm), len(P), literal, stuck, len(pool)))
            pool += Np + Nm + Dp + Dm + P + Z
        print("static const ModdivCase MODDIV_%s[] = {\n%s\n};" % (tag, "\n".join(table)))
        print("static const uint64_t MODDIV_POOL_%s[][4] = {\n%s\n};\n" % (tag, "\n".join("    %s," % words(v) for v in pool)))


if __name__ == "__main__":
    main()
