// One pairing product check spread over a group of lanes of one wave (pairing_wave.hip: k_pairing_check_wave; pm_verify_batch2 with
// PM_VERIFY_PAIRING_DEVICE_WAVE; DESIGN.md "Batch verification").  This header is the decomposition, stated once as PM_HD text: the
// kernel calls it with its lane index, tests/native/pairing_wave_selftest.cpp runs the same text lane after lane on the host against
// Tower<C> (pairing.cuh) and xyzz_mul_words (ec.cuh).  The algorithm is Tower<C>::product_is_one's, step for step.
//
// An Fq12 is an IMAGE: its six Fq2 coefficients over w (w^6 = xi), c[i] at w^i.  In the tower's terms
//     c[0] = c0.c0   c[1] = c1.c0   c[2] = c0.c1   c[3] = c1.c1   c[4] = c0.c2   c[5] = c1.c2          (v = w^2).
// A group is WAVE_GROUP = 36 lanes; the lanes past 64 / 36 * 36 of a wave idle along.
//   product  a b : lane 6 i + j forms a.c[i] b.c[j] (one Karatsuba Fq2 product); coefficient c of the result is the sum of the six
//                  products with i + j = c, plus xi times the sum of those with i + j = c + 6.  Lane c < 6 collects coefficient c.
//   squaring     : the same routine with b = a.
//   line         : a line has three non-zero coefficients (pairing.cuh "G2"), at w^0, w^1, w^3 (D-type, BN254) or w^0, w^2, w^3
//                  (M-type, BLS12-381): slot s < 3 at position LINE_POS[s].  Lane 3 i + s < 18 forms a.c[i] line[s]; collection as
//                  above with j = LINE_POS[s].  Lane s < 3 forms slot s from the table's line and the G1 point; a pair whose G1 point
//                  is infinity has the line 1 (a select, not a branch: groups of one wave may differ).
//   Frobenius    : in this basis a^p is coefficient-wise, conj(c[i]) gamma_i: lane i < 6 has no partner.
//   conjugate    : a^(p^6) negates the odd coefficients.
//   == 1         : lane i < 6 compares its coefficient; the group's six verdicts meet in one ballot.
// Fq2 products are the dense Montgomery product of field.cuh (on the device that is the 28-bit-limb product already, with canonical
// results), NOT fq28.cuh's internal radix: the line tables and Consts of pairing_prepare are dense and stay as they are, and a second
// radix would cost a conversion per line.  Every value is canonical after every step, so images compare equal to the tower's.
//
// The prelude of a tree node's check is (-g) G for this call's G: a table of d 2^(4 t) G, t < 64, d = 1 .. 15 (fixed_base_build, host,
// once per call), lane l < 32 adds the entries of windows 2 l and 2 l + 1, and a tree of complete additions (stride 16, 8, 4, 2, 1:
// lane l < stride adds slot l + stride into slot l) sums them.
#pragma once
#include "pairing.cuh"

namespace pm {

constexpr int WAVE_GROUP = 36;                                  // lanes a check: one per product a.c[i] b.c[j]
constexpr int WAVE_CHECKS = 64 / WAVE_GROUP;                    // checks a wave
constexpr int WAVE_FB_WINDOWS = 64, WAVE_FB_DIGITS = 15;        // 4-bit windows of a 256-bit scalar
constexpr int WAVE_FB_LANES = WAVE_FB_WINDOWS / 2;              // two windows a lane
constexpr int WAVE_FB_ENTRIES = WAVE_FB_WINDOWS * WAVE_FB_DIGITS;

template <class C>
struct WaveTower {
    typedef Tower<C> T;
    typedef typename T::Q Q;
    typedef typename T::Fq Fq;
    typedef typename T::PP PP;
    typedef typename T::Fq2 Fq2;
    typedef typename T::Fq12 Fq12;
    typedef typename T::Line Line;
    typedef typename T::Consts Consts;
    struct Image { Fq2 c[6]; };

    static Image from_tower(const Fq12 &f) { return Image{{f.c0.c0, f.c1.c0, f.c0.c1, f.c1.c1, f.c0.c2, f.c1.c2}}; }
    PM_HD static Fq12 to_tower(const Image &a) {
        return Fq12{typename T::Fq6{a.c[0], a.c[2], a.c[4]}, typename T::Fq6{a.c[1], a.c[3], a.c[5]}};
    }
    PM_HD static void store_tower(const Fq12 &f, Image &a) {
        a.c[0] = f.c0.c0; a.c[1] = f.c1.c0; a.c[2] = f.c0.c1; a.c[3] = f.c1.c1; a.c[4] = f.c0.c2; a.c[5] = f.c1.c2;
    }

    // T::mul2, inlined: the kernel's product site must not pass its operands through a call frame
    PM_HD static Fq2 mul2i(const Fq2 &a, const Fq2 &b) {
        const Fq t0 = mul<Q>(a.c0, b.c0), t1 = mul<Q>(a.c1, b.c1);
        const Fq m = mul<Q>(add<Q>(a.c0, a.c1), add<Q>(b.c0, b.c1));
        return Fq2{sub<Q>(t0, t1), sub<Q>(sub<Q>(m, t0), t1)};
    }

    // ------------------------------------------------------------------------------------------------ products and collection
    // the second operand has `cols` slots: 6 coefficients, or the 3 slots of a line; slot j sits at w^slot_pos(line, j)
    PM_HD static int cols(bool line) { return line ? 3 : 6; }
    PM_HD static int products(bool line) { return 6 * cols(line); }
    PM_HD static int slot_pos(bool line, int j) { return !line ? j : j == 0 ? 0 : j == 2 ? 3 : PP::D_TWIST ? 1 : 2; }
    // lane < products(line): a.c[lane / cols] b.c[lane % cols]
    PM_HD static Fq2 product(int lane, const Image &a, const Image &b, bool line) {
        const int n = cols(line);
        return mul2i(a.c[lane / n], b.c[lane % n]);
    }
    // lane c < 6: coefficient c of the result from the products of all lanes; the products past w^5 wrap and pick up xi
    PM_HD static Fq2 collect(int c, const Fq2 *prod, bool line) {
        const int n = cols(line);
        Fq2 lo = T::zero2(), hi = T::zero2();
#pragma unroll 1
        for (int j = 0; j < n; ++j) {
            const int i = c - slot_pos(line, j);
            const Fq2 t = prod[(i < 0 ? i + 6 : i) * n + j];
            if (i < 0) hi = T::add2(hi, t);
            else lo = T::add2(lo, t);
        }
        return T::add2(lo, T::mul_xi(hi));
    }

    // ------------------------------------------------------------------------------------------------------- per-coefficient
    PM_HD static Fq2 one_coeff(int c) { return c == 0 ? T::one2() : T::zero2(); }
    PM_HD static bool is_one_coeff(int c, const Fq2 &a) { return c == 0 ? T::eq2(a, T::one2()) : T::is_zero2(a); }
    PM_HD static Fq2 conj_coeff(int c, const Fq2 &a) { return (c & 1) ? T::neg2(a) : a; }
    PM_HD static Fq2 frob_coeff(int c, const Fq2 &a, const Consts &K) {
        const Fq2 t = T::conj2(a);
        return c == 0 ? t : mul2i(t, K.gamma[c - 1]);
    }
    // slot s < 3 of the line L at the G1 point P (T::mul_line's line); P = O: the line 1
    PM_HD static Fq2 line_coeff(int s, const Line &L, const Affine<C> &P) {
        const bool inf = P.is_inf();
        const Fq2 y{P.y, Fq::zero()};
        Fq2 r;
        if (s == 1) r = Fq2{mul<Q>(L.a.c0, P.x), mul<Q>(L.a.c1, P.x)};
        else r = (s == 0) == PP::D_TWIST ? y : L.b;             // D-type: y, a x, b    M-type: b, a x, y
        return inf ? one_coeff(s) : r;
    }

    // ------------------------------------------------------------------------------------------------- fixed-base (-g) G
    // out: WAVE_FB_ENTRIES points, d 2^(4 t) G at [15 t + d - 1], XYZZ in standard Montgomery form; G = O gives identities
    static void fixed_base_build(const Affine<C> &G, XYZZ<C> *out) {
        XYZZ<C> base = XYZZ<C>::from_affine(G);
        for (int t = 0; t < WAVE_FB_WINDOWS; ++t) {
            XYZZ<C> *row = out + t * WAVE_FB_DIGITS;
            row[0] = base;
            for (int d = 2; d <= WAVE_FB_DIGITS; ++d) row[d - 1] = xyzz_add<C>(row[d - 2], base);
            base = xyzz_dbl<C>(row[7]);                          // 16 B = 2 (8 B)
        }
    }
    PM_HD static unsigned digit(const uint32_t *k, int t) { return (k[t >> 3] >> (4 * (t & 7))) & 15u; }
    // lane l < WAVE_FB_LANES: the entries of windows 2 l and 2 l + 1 of the scalar k (8 canonical words), added
    PM_HD static XYZZ<C> fixed_base_lane(int l, const XYZZ<C> *table, const uint32_t *k) {
        const unsigned d0 = digit(k, 2 * l), d1 = digit(k, 2 * l + 1);
        const XYZZ<C> a = d0 ? table[(2 * l) * WAVE_FB_DIGITS + d0 - 1] : XYZZ<C>::identity();
        const XYZZ<C> b = d1 ? table[(2 * l + 1) * WAVE_FB_DIGITS + d1 - 1] : XYZZ<C>::identity();
        return xyzz_add<C>(a, b);
    }
    // one level of the sum over the lanes' slots: lane l < stride, stride = WAVE_FB_LANES / 2, .., 1
    PM_HD static void fixed_base_tree_step(int l, int stride, XYZZ<C> *slots) { slots[l] = xyzz_add<C>(slots[l], slots[l + stride]); }
};

}  // namespace pm
