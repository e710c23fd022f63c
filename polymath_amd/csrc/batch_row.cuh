// What differs from proof to proof in phases 2 and 3 of the prover, as plain PM_HD code: the numerator's constants, its reduced-radix
// multipliers, and the BatchRow record a group of proofs keeps per row in device memory.  The host builds the records of the host-glue
// prover with these functions (prove.hip, prove_sharded.hip, prove_batch.hip), k_glue_x2 of prove_glue.hip builds them in a lane; a
// host compiler reads this file too (tests/native/prover_glue_selftest.cpp).
#pragma once
#include "field.cuh"
#include "fq28.cuh"

namespace pm {

constexpr unsigned DIV_L = 16;      // 16 puts 20 K waves on the chip at 2^20 (32: 10 K, half of its wave slots idle): 0.98 -> 0.90 ms

template <class P>
struct NumConsts {
    Fp<P> x2, r0, r1, x2r0, x2r1, b2[3], two_x2_r0, two_x2_r1, minus_const;
};

// the constants of the numerator (prover.rs:145-197) from the challenges and r_a
template <class P>
PM_HD NumConsts<P> make_num_consts(const Fp<P> &x2, const Fp<P> rah[2], const Fp<P> &a_at, const Fp<P> &c_at) {
    NumConsts<P> nc;
    nc.x2 = x2;
    nc.r0 = rah[0];
    nc.r1 = rah[1];
    nc.x2r0 = mul<P>(x2, rah[0]);
    nc.x2r1 = mul<P>(x2, rah[1]);
    nc.b2[0] = add<P>(rah[0], mul<P>(x2, sqr<P>(rah[0])));
    nc.b2[1] = add<P>(rah[1], mul<P>(x2, dbl<P>(mul<P>(rah[0], rah[1]))));
    nc.b2[2] = mul<P>(x2, sqr<P>(rah[1]));
    nc.two_x2_r0 = dbl<P>(nc.x2r0);
    nc.two_x2_r1 = dbl<P>(nc.x2r1);
    nc.minus_const = neg<P>(add<P>(a_at, mul<P>(x2, c_at)));
    return nc;
}

// Round 5: the two kernels that walk the numerator -- k_div_level0 and k_div_expand0, 0.77 of the scan's 0.89 ms -- run their Horner
// chains in REDUCED RADIX (fq28.cuh: 9 limbs of 29 bits), as the transform tiles do: the multipliers x1, x2, 2 x2 r_a are handed over
// in the internal Montgomery form (value 2^261 mod p), so that f28_mul(standard-form value, multiplier) is again a standard-form
// value, sums are limb-wise, and a dense canonical element is only rebuilt where one is STORED.  The dense product mul<P> unpacks both
// operands and shifts / reduces / packs its result every time: ~370 instructions for 162 multiplier operations against ~200.
// Values are the same residues, the stored elements the same canonical words.
template <class RR>
struct NumMul28 {
    F28<RR> x1, x2, two_x2_r0, two_x2_r1;      // internal form, canonical, tight limbs
};
template <class P>
PM_HD NumMul28<typename Radix28<P>::RR> make_num_mul28(const Fp<P> &x1, const NumConsts<P> &nc) {
    typedef typename Radix28<P>::RR RR;
    Fp<P> k;
    for (int i = 0; i < P::N; ++i) k.l[i] = RR::STD2INT[i];
    NumMul28<RR> m;
    m.x1 = f28_unpack<RR>(mul<P>(x1, k).l);
    m.x2 = f28_unpack<RR>(mul<P>(nc.x2, k).l);
    m.two_x2_r0 = f28_unpack<RR>(mul<P>(nc.two_x2_r0, k).l);
    m.two_x2_r1 = f28_unpack<RR>(mul<P>(nc.two_x2_r1, k).l);
    return m;
}

// one record per row in device memory (uniform per workgroup: scalar loads)
template <class P>
struct BatchRow {
    Fp<P> x1;
    NumConsts<P> nc;
    NumMul28<typename Radix28<P>::RR> m28;
    Fp<P> xp[8];          // xp[l] = x1^(DIV_L^l): the multiplier of level l of the division scan
};

// phase 3's record of one proof (phase 2 reads x1 alone); R arrives zeroed, xp above `levels` stays zero
template <class P>
PM_HD void fill_batch_row(BatchRow<P> &R, const Fp<P> &x1, const Fp<P> &x2, const Fp<P> ra[2], const Fp<P> &a_at, const Fp<P> &c_at, int levels) {
    R.x1 = x1;
    R.nc = make_num_consts<P>(x2, ra, a_at, c_at);
    R.m28 = make_num_mul28<P>(R.x1, R.nc);
    R.xp[0] = R.x1;
    for (int l = 1; l <= levels; ++l) R.xp[l] = pow_u64<P>(R.xp[l - 1], DIV_L);
}

}  // namespace pm
