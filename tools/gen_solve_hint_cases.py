"""Writes solve_hint_cases.hpp, which is not committed: the literals of tests/native/solve_hint_selftest.cpp, computed with Python integers
(divmod; polymath_amd.circuits.modmul_values for the gadgets).  Per curve a table of long divisions -- limb width, the limbs of
dividend and divisor as field elements, whether the step sticks, and the limbs of quotient and remainder -- and the operands and
remainders of the modular multiplications the program builds as circuits.

    python tools/gen_solve_hint_cases.py > DIR/solve_hint_cases.hpp        and build the program with -I DIR
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polymath_amd import circuits as PC  # noqa: E402

R = {"BLS": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
     "BN": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001}
SECP = 2 ** 256 - 2 ** 32 - 977
P381 = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB


def limbs_of(value, n, count):
    return [(value >> (n * i)) & ((1 << n) - 1) for i in range(count)]


def cases(r):
    g = PC.SplitMix64(0x6C6F6E67646976)
    rnd = lambda bits: sum(g.next_u64() << (64 * i) for i in range(-(-bits // 64))) & ((1 << bits) - 1)
    out = []   # (name, n, kq, kr, D limbs, E limbs, literal)

    def add(name, n, kq, kr, D, E, literal=0):
        assert all(0 <= v < r for v in D + E), name
        out.append((name, n, kq, kr, list(D), list(E), literal))

    full = (1 << 128) - 1
    add("D = 0", 64, 4, 4, [0] * 8, limbs_of(SECP, 64, 4))
    add("D < E", 64, 4, 4, limbs_of(SECP - 1, 64, 4) + [0] * 3, limbs_of(SECP, 64, 4), 1)
    add("E = 1", 64, 8, 1, limbs_of(rnd(512), 64, 8), [1])
    add("D = 2^1024 - 1, E = 3", 128, 8, 1, [full] * 8, [3])
    add("D = 2^1024 - 1, E = 2^512 - 1", 128, 5, 4, [full] * 8, [full] * 4)
    add("E = 2^512 - 1, literal", 128, 4, 4, limbs_of(rnd(1000), 128, 8), [full] * 4, 1)
    add("D = E", 86, 1, 3, limbs_of(SECP, 86, 3), limbs_of(SECP, 86, 3))
    for n, kD, kE in ((1, 32, 16), (32, 16, 8), (64, 8, 4), (86, 5, 3), (128, 7, 4)):
        D, E = rnd(n * kD), rnd(n * kE) | 1
        q = D // E
        kq = max(1, -(-q.bit_length() // n))
        add("n = %d" % n, n, min(kq, 32), kE, limbs_of(D, n, kD), limbs_of(E, n, kE))
        add("n = %d, literal" % n, n, min(kq, 32), kE, limbs_of(D, n, kD), limbs_of(E, n, kE), 1)
    # un-normalised limbs: every limb a whole field element, so that carries run across several limbs
    add("n = 1, 32 limbs of 250 bits", 1, 32, 16, [rnd(250) for _ in range(32)], [rnd(200) | 1 for _ in range(16)])
    add("n = 64, limbs of 200 bits, all ones", 64, 7, 5, [(1 << 200) - 1] * 5, [(1 << 130) - 1] * 3)
    add("n = 86, the limbs of a no-carry product", 86, 3, 3, PC.limb_product(limbs_of(rnd(258), 86, 3), limbs_of(rnd(258), 86, 3), r), limbs_of(SECP, 86, 3), 1)
    add("a limb equal to r - 1", 64, 8, 4, [r - 1, 5, r - 1, 0, r - 1], [r - 1, 1])
    add("a divisor limb equal to r - 1, literal", 32, 16, 8, [r - 1] * 9, [7, r - 1], 1)
    # the five stuck conditions, each at its boundary and one below
    add("stuck: E = 0", 64, 4, 4, limbs_of(rnd(300), 64, 8), [0, 0, 0])
    add("stuck: E = 0, literal", 64, 4, 4, limbs_of(rnd(300), 64, 8), [0], 1)
    add("D = 2^1024 exactly", 128, 8, 1, [0] * 7 + [1 << 128], [1 << 127])
    add("D = 2^1024 by carries", 128, 8, 1, [1 << 128] + [full] * 7, [1 << 127])     # 2^128 + (2^1024 - 2^128)
    add("D = 2^1024 - 1, E = 2^127", 128, 8, 1, [full] * 8, [1 << 127])
    add("E = 2^512 exactly", 128, 4, 4, limbs_of(rnd(900), 128, 8), [0, 0, 0, 1 << 128])
    add("E = 2^512 exactly, literal", 128, 4, 4, limbs_of(rnd(900), 128, 8), [0, 0, 0, 1 << 128], 1)
    E = rnd(200) | 1
    add("q = 2^(n kq)", 64, 3, 4, limbs_of(E << 192, 64, 8), limbs_of(E, 64, 4))
    add("q = 2^(n kq) - 1", 64, 3, 4, limbs_of((E << 192) - 1, 64, 8), limbs_of(E, 64, 4))
    E = (1 << 172) + 1
    add("rem = 2^(n kr)", 86, 4, 2, limbs_of(12345 * E + (1 << 172), 86, 4), limbs_of(E, 86, 3))
    add("rem = 2^(n kr) - 1", 86, 4, 2, limbs_of(12345 * E + (1 << 172) - 1, 86, 4), limbs_of(E, 86, 3))
    rows = []
    for name, n, kq, kr, D, E, literal in out:
        Dv, Ev = sum(v << (n * j) for j, v in enumerate(D)), sum(v << (n * j) for j, v in enumerate(E))
        stuck = Ev == 0 or Dv >= 1 << 1024 or Ev >= 1 << 512
        q, rem = (0, 0) if stuck else divmod(Dv, Ev)
        stuck = stuck or q >= 1 << (n * kq) or rem >= 1 << (n * kr)
        if stuck:
            q = rem = 0
        rows.append((name, n, kq, kr, D, E, literal, int(stuck), limbs_of(q, n, kq), limbs_of(rem, n, kr)))
    return rows


def words(v):
    return "{%s}" % ", ".join("0x%016xull" % ((v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF) for i in range(4))


def gadgets(r):
    """(n, l, modulus, a, b) of the LimbModMul cases and (n, l, modulus, x0, b, steps) of the chains, with the remainders' limbs"""
    g = PC.SplitMix64(0x6D6F646D756C)
    rnd = lambda bits: sum(g.next_u64() << (64 * i) for i in range(-(-bits // 64))) & ((1 << bits) - 1)
    muls = []
    for n, l, modulus, bits in ((64, 4, SECP, 256), (86, 3, SECP, 256), (128, 4, P381, 124), (16, 2, 65521 * 65519, 31)):
        for _ in range(2):
            a = rnd(bits) % modulus if bits == 256 else sum(rnd(bits) << (n * i) for i in range(l - 1))
            b = rnd(bits) % modulus if bits == 256 else sum(rnd(bits) << (n * i) for i in range(l - 1))
            muls.append((n, l, limbs_of(modulus, n, l), limbs_of(a, n, l), limbs_of(b, n, l), limbs_of(a * b % modulus, n, l)))
            PC.modmul_values(muls[-1][3], muls[-1][4], muls[-1][2], n, r)      # asserts that no product limb reaches r
    chains = []
    for n, l, modulus, steps in ((64, 4, SECP, 4), (86, 3, SECP, 3)):
        x0, b = rnd(250), rnd(255)
        chains.append((n, l, steps, limbs_of(modulus, n, l), limbs_of(x0, n, l), limbs_of(b, n, l), limbs_of(x0 * pow(b, steps, modulus) % modulus, n, l)))
    return muls, chains


def main():
    print("// Generated by tools/gen_solve_hint_cases.py with Python integers; do not edit.  The literals of solve_hint_selftest.cpp.")
    print("#pragma once\n#include <stdint.h>\n")
    print("struct LongdivCase { const char *name; uint32_t n, kq, kr, kD, kE, literal, stuck, at; };   // at: its first element in the pool: D, E, q, rem")
    print("struct ModMulCase { uint32_t n, l, steps, at; };   // at: its first element in the pool: p, a (x0), b, rem (the last x), l limbs each\n")
    for tag, r in R.items():
        pool, table = [], []
        for name, n, kq, kr, D, E, literal, stuck, q, rem in cases(r):
            table.append('    {"%s", %d, %d, %d, %d, %d, %d, %d, %d},' % (name, n, kq, kr, len(D), len(E), literal, stuck, len(pool)))
            pool += D + E + q + rem
        print("static const LongdivCase LONGDIV_%s[] = {\n%s\n};" % (tag, "\n".join(table)))
        print("static const uint64_t LONGDIV_POOL_%s[][4] = {\n%s\n};\n" % (tag, "\n".join("    %s," % words(v) for v in pool)))
        muls, chains = gadgets(r)
        pool, table = [], []
        for n, l, p, a, b, rem in muls:
            table.append("    {%d, %d, 0, %d}," % (n, l, len(pool)))
            pool += p + a + b + rem
        for n, l, steps, p, x0, b, rem in chains:
            table.append("    {%d, %d, %d, %d}," % (n, l, steps, len(pool)))
            pool += p + x0 + b + rem
        print("static const ModMulCase MODMUL_%s[] = {\n%s\n};" % (tag, "\n".join(table)))
        print("static const uint64_t MODMUL_POOL_%s[][4] = {\n%s\n};\n" % (tag, "\n".join("    %s," % words(v) for v in pool)))


if __name__ == "__main__":
    main()
