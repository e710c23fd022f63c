// The square root in the two scalar fields, for the witness solver's square-root step (solve_steps.cuh: solve_sqrt; solve.hip:
// k_solve_sqrt).  ONE text for device and host, like divrem.cuh: the kernels call it per (step, assignment) through
// the step bodies, and the CPU self-test (tests/native/solve_sqrt_selftest.cpp) executes it on the host field type.
//
// Tonelli-Shanks with a trip count that does NOT depend on the operand: the lanes of a wave hold different assignments, and with a
// 2-adicity of 32 (BLS12-381) / 28 (BN254) the textbook loops -- "square until one", "repeat while t != 1" -- would diverge.  This is
// the constant-time form of RFC 9380, appendix I.4 (sqrt_ts_ct), with selects where it has CMOVs.  With r - 1 = 2^s t, t odd:
//   z = c^((t - 1) / 2)            the exponent is MOD >> (s + 1); square-and-multiply over its bitlength(r) - s - 1 bits, which are the
//                                  same in every lane (the branch on an exponent bit is uniform)
//   t = z z c,  z = z c            c^t (in the 2^s-torsion) and c^((t + 1) / 2): z^2 = c t
//   w = ROOT                       the 2^s-th root of unity the transforms use (g^t, g = 7 / 5 the generator): a non-residue to the t
//   for i = s, s - 1, ..., 2:      b = t^(2^(i - 2)); where b != 1: z = z w, t = t w^2; w = w^2 in every lane
// 222 / 225 squarings in the exponentiation and 558 / 432 multiplications in the loop nest.  For a residue the loops end with t = 1 and
// z^2 = c; for a non-residue t ends as -1, so the final comparison z^2 == c IS the residue test and no Euler-criterion exponentiation
// is run.  c = 0 gives z = 0.  The SMALLER root -- canonical integer <= (r - 1) / 2, what circom's sqrt returns -- is then selected
// under a mask: from_mont, one comparison with (r - 1) / 2 = MOD >> 1, one masked negation.
// Both outer loops stay rolled (a body is four inlined Montgomery products; unrolled they would be ~100 of them), no register array is
// indexed by a run-time value, and five field elements are live across the loop nest (c, z, t, b, w: 40 VGPRs).  Plain C++, no inline
// assembly.
#pragma once
#include "field.cuh"

namespace pm {

// r - 1 = 2^S t: S and the primitive 2^S-th root of unity g^t in Montgomery form, per scalar field
template <class P>
struct SqrtField;
template <>
struct SqrtField<BlsFrP> {
    typedef BlsCurve C;
};
template <>
struct SqrtField<BnFrP> {
    typedef BnCurve C;
};

// word w of MOD >> sh, for compile-time w and sh (0 < sh % 32 is not assumed)
template <class P>
PM_HD constexpr uint32_t mod_shifted_word(int w, int sh) {
    const int lo = w + sh / 32, bit = sh % 32;
    const uint32_t a = lo < P::N ? P::MOD[lo] : 0u, b = lo + 1 < P::N ? P::MOD[lo + 1] : 0u;
    return bit ? (a >> bit) | (b << (32 - bit)) : a;
}

// take_x ? x : y per limb, under a mask: no branch on the operands
template <class P>
PM_HD Fp<P> fr_select(bool take_x, const Fp<P> &x, const Fp<P> &y) {
    const uint32_t mask = 0u - (uint32_t)take_x;
    Fp<P> r;
#pragma unroll
    for (int i = 0; i < P::N; ++i) r.l[i] = (x.l[i] & mask) | (y.l[i] & ~mask);
    return r;
}

// c (Montgomery form) a square, 0 included: *root = the root whose canonical integer is <= (r - 1) / 2, Montgomery form, -> true.
// c a non-residue: -> false and nothing written.
template <class P>
PM_HD_COLD bool fr_sqrt(const Fp<P> &operand, Fp<P> *root) {
    typedef typename SqrtField<P>::C C;
    const Fp<P> c = operand;      // read once: the caller's copy lies in memory (a real call), the loops below work on registers
    static_assert(P::N == 8, "four 64-bit words");
    constexpr int N = P::N, S = C::TWO_ADICITY, EXP_BITS = P::BITS - S - 1;   // bitlength of (t - 1) / 2 = MOD >> (S + 1)
    // z = c^((t - 1) / 2), most significant bit first
    Fp<P> z = Fp<P>::one();
#pragma unroll 1
    for (int k = EXP_BITS - 1; k >= 0; --k) {
        uint32_t word = 0;
#pragma unroll
        for (int w = 0; w < N; ++w) word = (k >> 5) == w ? mod_shifted_word<P>(w, S + 1) : word;
        z = sqr<P>(z);
        if ((word >> (k & 31)) & 1u) z = mul<P>(z, c);      // the exponent is the same in every lane
    }
    Fp<P> t = mul<P>(sqr<P>(z), c);
    z = mul<P>(z, c);
    Fp<P> b = t, w;
#pragma unroll
    for (int i = 0; i < N; ++i) w.l[i] = C::ROOT_MONT[i];
    const Fp<P> one = Fp<P>::one();
#pragma unroll 1
    for (int i = S; i >= 2; --i) {
#pragma unroll 1
        for (int j = 1; j <= i - 2; ++j) b = sqr<P>(b);
        const bool e = b.eq(one);
        z = fr_select<P>(e, z, mul<P>(z, w));
        w = sqr<P>(w);
        t = fr_select<P>(e, t, mul<P>(t, w));
        b = t;
    }
    if (!sqr<P>(z).eq(c)) return false;
    // the smaller root: negate where the canonical integer exceeds (r - 1) / 2
    const Fp<P> zc = from_mont<P>(z);
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint64_t d = (uint64_t)mod_shifted_word<P>(i, 1) - zc.l[i] - borrow;
        borrow = (d >> 32) & 1;
    }
    *root = fr_select<P>(borrow != 0, sub<P>(Fp<P>::zero(), z), z);
    return true;
}

}  // namespace pm
