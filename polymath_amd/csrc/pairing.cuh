// Pairing product checks  prod_j e(P_j, Q_j) == 1  for BLS12-381 and BN254, one check per lane (pairing_batch.hip: k_pairing_check;
// DESIGN.md "Batch verification").  PM_HD like verify_batch.cuh: the same text runs under g++ in tests/native/pairing_selftest.cpp,
// against the oracle-pinned host pairing (host/pairing.hpp), which it agrees with value for value (see "exponent" below).
//
// Tower:   Fq2 = Fq[u]/(u^2 + 1),  Fq6 = Fq2[v]/(v^3 - xi),  Fq12 = Fq6[w]/(w^2 - v),  xi = 1 + u (BLS12-381) / 9 + u (BN254).
//          w^6 = xi, the w of host/pairing.hpp: sum_i a_i w^i with a_i = a + b u is host coefficient a - XI0 b at w^i, b at w^(i + 6).
// G2:      every G2 argument of a check is FIXED (it belongs to the verifying key), so the host walks the Miller loop once per call in
//          affine coordinates on the twist (prepare) and leaves one Line per step: a = -lambda, b = lambda x_T - y_T.  With the
//          untwist (x w^2, y w^3) (D-type, BN254) or (x / w^2, y / w^3) (M-type, BLS12-381) the line through T evaluated at the G1
//          point (xP, yP) is, up to factors in proper subfields (which the final exponentiation removes),
//              D-type:  yP + (a xP) w + b w^3            M-type:  b + (a xP) w^2 + yP w^3
//          three of six Fq2 coefficients, one of them in Fq.  No vertical lines, as in the host's loop.
// Loop:    |x| = 0xd201000000010000 (BLS12-381, no conjugation for x < 0: the host's loop has none either); 6x + 2 and the two
//          Frobenius steps pi(Q), -pi^2(Q) (BN254), which are two more lines of the table.  k pairs share the squaring of f.
//          A pair whose G1 point is infinity is skipped: it contributes 1.
// Exponent: the easy part f^((p^6 - 1)(p^2 + 1)) by conjugation, one inversion and Frobenius; the hard part (p^4 - p^2 + 1) / r by
//          an x-chain, inverses being conjugates from there on:
//              BN254    : exact,  p^3 + (6x^2 + 1) p^2 + (-36x^3 - 18x^2 - 12x + 1) p + (-36x^3 - 30x^2 - 18x - 2)
//              BLS12-381: m = 3 times it,  (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3
//          so final_exp gives e^m of the host's value with m = HARD_MULTIPLE = 1 (BN254) / 3 (BLS12-381); 3 does not divide r, so
//          e^3 == 1 iff e == 1.  Both identities are integer identities in x (checked with big integers, tests/test_native_pairing.py).
// Frobenius constants gamma_i = xi^(i (p - 1) / 6), i = 1..5, are derived on the host by exponentiation (make_consts) and handed to
// the lanes in device memory next to the line tables.
#pragma once
#include "ec.cuh"

namespace pm {

template <class C>
struct PairingParams;
template <>
struct PairingParams<BlsCurve> {
    static constexpr unsigned XI0 = 1;
    static constexpr bool D_TWIST = false, FROBENIUS_STEPS = false, X_NEGATIVE = true;
    static constexpr uint64_t LOOP_LO = 0xd201000000010000ull, LOOP_HI = 0, X_ABS = 0xd201000000010000ull;
    static constexpr int LOOP_TOP = 63, LINES = 63 + 5;        // doublings + set bits below the top one
    static constexpr unsigned HARD_MULTIPLE = 3;
};
template <>
struct PairingParams<BnCurve> {
    static constexpr unsigned XI0 = 9;
    static constexpr bool D_TWIST = true, FROBENIUS_STEPS = true, X_NEGATIVE = false;
    static constexpr uint64_t LOOP_LO = 0x9d797039be763ba8ull, LOOP_HI = 1, X_ABS = 0x44e992b44a6909f1ull;   // 6x + 2, x
    static constexpr int LOOP_TOP = 64, LINES = 64 + 36 + 2;
    static constexpr unsigned HARD_MULTIPLE = 1;
};

constexpr int PAIRING_MAX_PAIRS = 4;

template <class C>
struct Tower {
    typedef typename C::FqP Q;
    typedef Fp<Q> Fq;
    typedef PairingParams<C> PP;
    struct Fq2 { Fq c0, c1; };
    struct Fq6 { Fq2 c0, c1, c2; };
    struct Fq12 { Fq6 c0, c1; };
    struct Line { Fq2 a, b; };
    struct Consts { Fq2 gamma[5]; };
    struct G2Affine { Fq2 x, y; };

    PM_HD static bool loop_bit(int i) { return i < 64 ? (PP::LOOP_LO >> i) & 1 : (PP::LOOP_HI >> (i - 64)) & 1; }

    // ---------------------------------------------------------------------------------------------------------------- Fq2
    PM_HD static Fq2 zero2() { return Fq2{Fq::zero(), Fq::zero()}; }
    PM_HD static Fq2 one2() { return Fq2{Fq::one(), Fq::zero()}; }
    PM_HD static bool is_zero2(const Fq2 &a) { return a.c0.is_zero() && a.c1.is_zero(); }
    PM_HD static bool eq2(const Fq2 &a, const Fq2 &b) { return a.c0.eq(b.c0) && a.c1.eq(b.c1); }
    PM_HD static Fq2 add2(const Fq2 &a, const Fq2 &b) { return Fq2{add<Q>(a.c0, b.c0), add<Q>(a.c1, b.c1)}; }
    PM_HD static Fq2 sub2(const Fq2 &a, const Fq2 &b) { return Fq2{sub<Q>(a.c0, b.c0), sub<Q>(a.c1, b.c1)}; }
    PM_HD static Fq2 neg2(const Fq2 &a) { return Fq2{neg<Q>(a.c0), neg<Q>(a.c1)}; }
    PM_HD static Fq2 conj2(const Fq2 &a) { return Fq2{a.c0, neg<Q>(a.c1)}; }
    PM_HD_COLD static Fq2 mul2(const Fq2 &a, const Fq2 &b) {   // Karatsuba: 3 products
        const Fq t0 = mul<Q>(a.c0, b.c0), t1 = mul<Q>(a.c1, b.c1);
        const Fq m = mul<Q>(add<Q>(a.c0, a.c1), add<Q>(b.c0, b.c1));
        return Fq2{sub<Q>(t0, t1), sub<Q>(sub<Q>(m, t0), t1)};
    }
    PM_HD_COLD static Fq2 sqr2(const Fq2 &a) {
        const Fq t = mul<Q>(a.c0, a.c1);
        return Fq2{mul<Q>(add<Q>(a.c0, a.c1), sub<Q>(a.c0, a.c1)), add<Q>(t, t)};
    }
    PM_HD_COLD static Fq2 scale2(const Fq2 &a, const Fq &s) { return Fq2{mul<Q>(a.c0, s), mul<Q>(a.c1, s)}; }
    PM_HD static Fq times_xi0(const Fq &a) {
        if (PP::XI0 == 1) return a;
        const Fq a8 = dbl<Q>(dbl<Q>(dbl<Q>(a)));
        return add<Q>(a8, a);                                   // XI0 == 9
    }
    PM_HD static Fq2 mul_xi(const Fq2 &a) {                     // (a0 + a1 u)(XI0 + u)
        static_assert(PP::XI0 == 1 || PP::XI0 == 9, "xi = 1 + u or 9 + u");
        return Fq2{sub<Q>(times_xi0(a.c0), a.c1), add<Q>(a.c0, times_xi0(a.c1))};
    }
    PM_HD_COLD static Fq2 inv2(const Fq2 &a) {
        const Fq d = inverse<Q>(add<Q>(sqr<Q>(a.c0), sqr<Q>(a.c1)));
        return Fq2{mul<Q>(a.c0, d), neg<Q>(mul<Q>(a.c1, d))};
    }

    // ---------------------------------------------------------------------------------------------------------------- Fq6
    PM_HD static Fq6 add6(const Fq6 &a, const Fq6 &b) { return Fq6{add2(a.c0, b.c0), add2(a.c1, b.c1), add2(a.c2, b.c2)}; }
    PM_HD static Fq6 sub6(const Fq6 &a, const Fq6 &b) { return Fq6{sub2(a.c0, b.c0), sub2(a.c1, b.c1), sub2(a.c2, b.c2)}; }
    PM_HD static Fq6 neg6(const Fq6 &a) { return Fq6{neg2(a.c0), neg2(a.c1), neg2(a.c2)}; }
    PM_HD static Fq6 mul6_v(const Fq6 &a) { return Fq6{mul_xi(a.c2), a.c0, a.c1}; }
    PM_HD_COLD static Fq6 mul6(const Fq6 &a, const Fq6 &b) {
        const Fq2 t0 = mul2(a.c0, b.c0), t1 = mul2(a.c1, b.c1), t2 = mul2(a.c2, b.c2);
        const Fq2 m12 = mul2(add2(a.c1, a.c2), add2(b.c1, b.c2)), m01 = mul2(add2(a.c0, a.c1), add2(b.c0, b.c1));
        const Fq2 m02 = mul2(add2(a.c0, a.c2), add2(b.c0, b.c2));
        return Fq6{add2(t0, mul_xi(sub2(sub2(m12, t1), t2))), add2(sub2(sub2(m01, t0), t1), mul_xi(t2)), add2(sub2(sub2(m02, t0), t2), t1)};
    }
    // a (b0 + b1 v): the shape of a line's two halves
    PM_HD_COLD static Fq6 mul6_01(const Fq6 &a, const Fq2 &b0, const Fq2 &b1) {
        return Fq6{add2(mul2(a.c0, b0), mul_xi(mul2(a.c2, b1))), add2(mul2(a.c0, b1), mul2(a.c1, b0)), add2(mul2(a.c1, b1), mul2(a.c2, b0))};
    }
    PM_HD_COLD static Fq6 scale6(const Fq6 &a, const Fq &s) { return Fq6{scale2(a.c0, s), scale2(a.c1, s), scale2(a.c2, s)}; }
    PM_HD_COLD static Fq6 inv6(const Fq6 &a) {
        const Fq2 A = sub2(sqr2(a.c0), mul_xi(mul2(a.c1, a.c2))), B = sub2(mul_xi(sqr2(a.c2)), mul2(a.c0, a.c1));
        const Fq2 D = sub2(sqr2(a.c1), mul2(a.c0, a.c2));
        const Fq2 F = add2(mul2(a.c0, A), mul_xi(add2(mul2(a.c2, B), mul2(a.c1, D))));
        const Fq2 Fi = inv2(F);
        return Fq6{mul2(A, Fi), mul2(B, Fi), mul2(D, Fi)};
    }

    // --------------------------------------------------------------------------------------------------------------- Fq12
    PM_HD static Fq12 one12() {
        const Fq2 z = zero2();
        return Fq12{Fq6{one2(), z, z}, Fq6{z, z, z}};
    }
    PM_HD static bool is_one12(const Fq12 &a) {
        return eq2(a.c0.c0, one2()) && is_zero2(a.c0.c1) && is_zero2(a.c0.c2) && is_zero2(a.c1.c0) && is_zero2(a.c1.c1) && is_zero2(a.c1.c2);
    }
    PM_HD static bool eq12(const Fq12 &a, const Fq12 &b) {
        return eq2(a.c0.c0, b.c0.c0) && eq2(a.c0.c1, b.c0.c1) && eq2(a.c0.c2, b.c0.c2) && eq2(a.c1.c0, b.c1.c0) && eq2(a.c1.c1, b.c1.c1) &&
               eq2(a.c1.c2, b.c1.c2);
    }
    PM_HD static Fq12 conj12(const Fq12 &a) { return Fq12{a.c0, neg6(a.c1)}; }   // a^(p^6)
    PM_HD_COLD static Fq12 mul12(const Fq12 &a, const Fq12 &b) {
        const Fq6 t0 = mul6(a.c0, b.c0), t1 = mul6(a.c1, b.c1);
        const Fq6 m = mul6(add6(a.c0, a.c1), add6(b.c0, b.c1));
        return Fq12{add6(t0, mul6_v(t1)), sub6(sub6(m, t0), t1)};
    }
    PM_HD_COLD static Fq12 sqr12(const Fq12 &a) {
        const Fq6 t = mul6(a.c0, a.c1);
        const Fq6 m = mul6(add6(a.c0, a.c1), add6(a.c0, mul6_v(a.c1)));
        return Fq12{sub6(sub6(m, t), mul6_v(t)), add6(t, t)};
    }
    PM_HD_COLD static Fq12 inv12(const Fq12 &a) {
        const Fq6 di = inv6(sub6(mul6(a.c0, a.c0), mul6_v(mul6(a.c1, a.c1))));
        return Fq12{mul6(a.c0, di), neg6(mul6(a.c1, di))};
    }
    // a^p: coefficient i of w^i is conjugated and multiplied by gamma_i
    PM_HD_COLD static Fq12 frob12(const Fq12 &a, const Consts &K) {
        return Fq12{Fq6{conj2(a.c0.c0), mul2(conj2(a.c0.c1), K.gamma[1]), mul2(conj2(a.c0.c2), K.gamma[3])},
                    Fq6{mul2(conj2(a.c1.c0), K.gamma[0]), mul2(conj2(a.c1.c1), K.gamma[2]), mul2(conj2(a.c1.c2), K.gamma[4])}};
    }
    // f times the line L of the table at the G1 point P (finite)
    PM_HD_COLD static Fq12 mul_line(const Fq12 &f, const Line &L, const Affine<C> &P) {
        const Fq2 t = scale2(L.a, P.x);
        if (PP::D_TWIST) {                                      // yP + (t + b v) w
            const Fq6 lo = add6(scale6(f.c0, P.y), mul6_v(mul6_01(f.c1, t, L.b)));
            return Fq12{lo, add6(mul6_01(f.c0, t, L.b), scale6(f.c1, P.y))};
        }
        const Fq6 y0 = scale6(f.c0, P.y), y1 = scale6(f.c1, P.y);   // (b + t v) + (yP v) w
        const Fq6 lo = add6(mul6_01(f.c0, L.b, t), mul6_v(mul6_v(y1)));
        return Fq12{lo, add6(mul6_v(y0), mul6_01(f.c1, L.b, t))};
    }

    // tab: k tables of PP::LINES lines, pair j's at tab + j * PP::LINES; pairs: bit j clear = pair j is left out (its G2 point is O)
    PM_HD_COLD static Fq12 miller(const Line *tab, int k, unsigned pairs, const Affine<C> *P) {
        Fq12 f = one12();
        bool live[PAIRING_MAX_PAIRS];
        for (int j = 0; j < PAIRING_MAX_PAIRS; ++j) live[j] = j < k && ((pairs >> j) & 1u) && !P[j].is_inf();
        int idx = 0;
#pragma unroll 1
        for (int i = PP::LOOP_TOP - 1; i >= -1; --i) {
            // i == -1: the two Frobenius lines of BN254, taken as one more "doubling + addition" without the squaring
            if (i < 0 && !PP::FROBENIUS_STEPS) break;
            if (i >= 0) f = sqr12(f);
            const int steps = i < 0 || loop_bit(i) ? 2 : 1;
#pragma unroll 1
            for (int s = 0; s < steps; ++s, ++idx) {
#pragma unroll 1
                for (int j = 0; j < k; ++j)
                    if (live[j]) f = mul_line(f, tab[j * PP::LINES + idx], P[j]);
            }
        }
        return f;
    }

    // g^|x|, then the sign of x: only for g in the cyclotomic subgroup (after the easy part), where 1/g is the conjugate
    PM_HD_COLD static Fq12 pow_x(const Fq12 &g) {
        Fq12 acc = g;
#pragma unroll 1
        for (int b = 62; b >= 0; --b) {
            if (b == 62 && !(PP::X_ABS >> 63)) continue;        // a 63-bit x starts one bit lower
            acc = sqr12(acc);
            if ((PP::X_ABS >> b) & 1) acc = mul12(acc, g);
        }
        return PP::X_NEGATIVE ? conj12(acc) : acc;
    }
    PM_HD_COLD static Fq12 pow_small(const Fq12 &g, unsigned e) {   // 1 <= e < 64
        int top = 5;
        while (!((e >> top) & 1u)) --top;
        Fq12 acc = g;
#pragma unroll 1
        for (int b = top - 1; b >= 0; --b) {
            acc = sqr12(acc);
            if ((e >> b) & 1u) acc = mul12(acc, g);
        }
        return acc;
    }
    // f^(HARD_MULTIPLE (p^12 - 1) / r)
    PM_HD_COLD static Fq12 final_exp(const Fq12 &f0, const Consts &K) {
        Fq12 f = mul12(conj12(f0), inv12(f0));                  // ^(p^6 - 1)
        f = mul12(frob12(frob12(f, K), K), f);                  // ^(p^2 + 1)
        if (PP::FROBENIUS_STEPS) {                              // BN254
            const Fq12 fx = pow_x(f), fx2 = pow_x(fx), fx3 = pow_x(fx2);
            const Fq12 c36 = pow_small(fx3, 36);
            const Fq12 l0 = conj12(mul12(mul12(c36, pow_small(fx2, 30)), mul12(pow_small(fx, 18), sqr12(f))));
            const Fq12 l1 = mul12(conj12(mul12(mul12(c36, pow_small(fx2, 18)), pow_small(fx, 12))), f);
            const Fq12 l2 = mul12(pow_small(fx2, 6), f);
            Fq12 r = frob12(f, K);                              // Horner in p: ((f^p l2)^p l1)^p l0
            r = frob12(mul12(r, l2), K);
            r = frob12(mul12(r, l1), K);
            return mul12(r, l0);
        }
        Fq12 a = mul12(pow_x(f), conj12(f));                    // BLS12-381: ^(x - 1), twice
        a = mul12(pow_x(a), conj12(a));
        const Fq12 b = mul12(pow_x(a), frob12(a, K));           // ^(x + p)
        const Fq12 c = mul12(mul12(pow_x(pow_x(b)), frob12(frob12(b, K), K)), conj12(b));   // ^(x^2 + p^2 - 1)
        return mul12(c, mul12(sqr12(f), f));                    // f^3
    }
    PM_HD_COLD static bool product_is_one(const Line *tab, int k, unsigned pairs, const Affine<C> *P, const Consts &K) {
        return is_one12(final_exp(miller(tab, k, pairs, P), K));
    }

    // ------------------------------------------------------------------------------------------ host: constants, prepared G2
    static Fq2 pow2_limbs(const Fq2 &a, const uint32_t *e, int n) {
        Fq2 acc = one2();
        for (int i = n - 1; i >= 0; --i)
            for (int b = 31; b >= 0; --b) {
                acc = sqr2(acc);
                if ((e[i] >> b) & 1) acc = mul2(acc, a);
            }
        return acc;
    }
    static Fq2 xi() { return Fq2{from_u64<Q>(PP::XI0), Fq::one()}; }
    static Consts make_consts() {
        uint32_t e[Q::N];                                       // (p - 1) / 6: p = 1 mod 6 on both curves
        uint64_t rem = 0;
        for (int i = Q::N - 1; i >= 0; --i) {
            const uint64_t cur = (rem << 32) | (Q::MOD[i] - (i == 0 ? 1u : 0u));
            e[i] = (uint32_t)(cur / 6);
            rem = cur % 6;
        }
        Consts K;
        K.gamma[0] = pow2_limbs(xi(), e, Q::N);
        for (int i = 1; i < 5; ++i) K.gamma[i] = mul2(K.gamma[i - 1], K.gamma[0]);
        return K;
    }
    static Fq2 twist_b() {                                      // y^2 = x^3 + b': b / xi (D-type) or b xi (M-type)
        Fq2 cb = zero2();
        for (int i = 0; i < Q::N; ++i) cb.c0.l[i] = C::B_MONT[i];
        return PP::D_TWIST ? mul2(cb, inv2(xi())) : mul_xi(cb);
    }
    static bool g2_on_twist(const G2Affine &A) { return eq2(sqr2(A.y), add2(mul2(sqr2(A.x), A.x), twist_b())); }
    // the line through T with slope m, then T <- the third point
    static Line line_and_step(G2Affine &T, const Fq2 &m, const Fq2 &other_x) {
        const Line L{neg2(m), sub2(mul2(m, T.x), T.y)};
        const Fq2 x3 = sub2(sub2(sqr2(m), T.x), other_x);
        T = G2Affine{x3, sub2(mul2(m, sub2(T.x, x3)), T.y)};
        return L;
    }
    static Line add_step(G2Affine &T, const G2Affine &A) { return line_and_step(T, mul2(sub2(A.y, T.y), inv2(sub2(A.x, T.x))), A.x); }
    static Line dbl_step(G2Affine &T) {
        const Fq2 x2 = sqr2(T.x);
        return line_and_step(T, mul2(add2(add2(x2, x2), x2), inv2(add2(T.y, T.y))), T.x);
    }
    // out: PP::LINES lines.  A point outside the prime-order subgroup gives lines of no meaning, never a fault (1 / 0 is 0 here).
    static void prepare(const G2Affine &A, const Consts &K, Line *out) {
        G2Affine T = A;
        int idx = 0;
        for (int i = PP::LOOP_TOP - 1; i >= 0; --i) {
            out[idx++] = dbl_step(T);
            if (loop_bit(i)) out[idx++] = add_step(T, A);
        }
        if (PP::FROBENIUS_STEPS) {                              // pi(x w^2, y w^3) = (conj(x) gamma_2 w^2, conj(y) gamma_3 w^3)
            const G2Affine A1{mul2(conj2(A.x), K.gamma[1]), mul2(conj2(A.y), K.gamma[2])};
            const G2Affine A2{mul2(conj2(A1.x), K.gamma[1]), neg2(mul2(conj2(A1.y), K.gamma[2]))};   // -pi^2(Q)
            out[idx++] = add_step(T, A1);
            out[idx++] = add_step(T, A2);
        }
    }
    // e(P, Q)^HARD_MULTIPLE of the host pairing, one pair (tests)
    static Fq12 pairing(const Affine<C> &P, const G2Affine &A, const Consts &K) {
        Line tab[PP::LINES];
        prepare(A, K, tab);
        return final_exp(miller(tab, 1, 1u, &P), K);
    }
};

}  // namespace pm
