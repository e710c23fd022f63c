// The markers of a partial assignment (marker_byte: THE marker test, for the solver and for both glue modes of the provers), the
// indicator step's value (indicator_of; solve_steps.cuh: solve_indicator) and the Euclidean division of canonical residues, for the
// witness solver's division step (solve.hip: k_solve_pattern; solve_steps.cuh: solve_divrem).  ONE set of routines
// for device and host: the kernels call them per (step, assignment) through the step bodies of solve_steps.cuh, and the CPU
// self-tests (tests/native/solve_selftest.hpp, the rig of the solve_*_selftest.cpp programs) execute plans through the same bodies on the
// host field type.
//
// Restoring shift-subtract on four 64-bit words with a FIXED trip count of 256: the 512-bit register (hi : lo) starts as (0 : a),
// every round shifts it left by one, subtracts d from hi on trial and keeps the difference under a mask; the quotient bit enters
// lo at the bottom, where the dividend's bits have left.  No branch depends on the operands, so the lanes of a wave do not diverge
// on operand size, and no register is indexed by a run-time value.  The round loop stays rolled (a round is ~50 instructions on
// 32-bit lanes; 256 rounds are about a tenth of one Fermat inversion).  Plain C++, no inline assembly.
#pragma once
#include "../host/solve_plan.hpp"
#include "field.cuh"

namespace pm {

// The pattern byte of a value of a partial assignment (include/polymath_hip.h): 1 for the unknown marker (every word all ones), 2 for
// the quotient marker (the same with the lowest bit clear), 3 for the indicator marker (the same with bit 64 clear), else 0 -- with
// both bits clear as well.  All three are >= r on both curves, so never a field element.  THE marker test: the solver's kernels, the
// host glue (host_prove.hip) and the device glue (prove_glue.hip) all ask this routine, on eight 32-bit limbs, little-endian.
// 4 for the square-root marker (every bit set except bit 192, the lowest bit of the top word; that word is 0xFFFF...FE, so the value
// is >= r on both curves as well): exactly ONE of the bits 0, 64 and 192 may be clear, and any two of them clear is no marker.
PM_HD uint8_t marker_byte_limbs(const uint32_t l[8]) {
    uint32_t a = (l[0] | 1u) & l[1] & (l[2] | 1u) & l[3] & l[4] & l[5] & (l[6] | 1u) & l[7];
    const uint32_t low = l[0] & 1u, mid = l[2] & 1u, high = l[6] & 1u;
    if (a != ~0u) return 0;
    return (low & mid & high) ? pmsolve::PATTERN_UNKNOWN
         : (mid & high)       ? pmsolve::PATTERN_QUOTIENT
         : (low & high)       ? pmsolve::PATTERN_INDICATOR
         : (low & mid)        ? pmsolve::PATTERN_SQRT : 0;
}
template <class P>
PM_HD uint8_t marker_byte(const Fp<P> &v) {
    static_assert(P::N == 8, "four 64-bit words");
    return marker_byte_limbs(v.l);
}

// The indicator step's value (solve.hip: solve_indicator): field one where the guard's known side is zero, else field zero.  One
// & mask, as solve_bits stores its bits: no table to select from and no branch on the operand.
template <class P>
PM_HD Fp<P> indicator_of(const Fp<P> &kz) {
    const uint32_t mask = 0u - (uint32_t)kz.is_zero();
    Fp<P> v;
#pragma unroll
    for (int w = 0; w < P::N; ++w) v.l[w] = P::ONE[w] & mask;
    return v;
}

// q = floor(a / d), rem = a mod d on unsigned 256-bit integers, little-endian words; any a, any d != 0 (the bit shifted out of hi
// is honoured, so d may use all 256 bits).  d == 0 gives q = 2^256 - 1: the caller tests for it.
PM_HD void divrem256(const uint64_t a[4], const uint64_t d[4], uint64_t q[4], uint64_t rem[4]) {
    uint64_t lo[4], hi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lo[j] = a[j];
        hi[j] = 0;
    }
#pragma unroll 1
    for (int round = 0; round < 256; ++round) {
        const uint64_t out = hi[3] >> 63;
#pragma unroll
        for (int j = 3; j > 0; --j) hi[j] = hi[j] << 1 | hi[j - 1] >> 63;
        hi[0] = hi[0] << 1 | lo[3] >> 63;
#pragma unroll
        for (int j = 3; j > 0; --j) lo[j] = lo[j] << 1 | lo[j - 1] >> 63;
        lo[0] <<= 1;
        uint64_t t[4], borrow = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t x = hi[j] - borrow;
            const uint64_t b1 = hi[j] < borrow;
            t[j] = x - d[j];
            borrow = b1 | (uint64_t)(x < d[j]);
        }
        const uint64_t take = out | (borrow ^ 1);   // 2 hi + bit >= d
        const uint64_t mask = 0 - take;
#pragma unroll
        for (int j = 0; j < 4; ++j) hi[j] = (t[j] & mask) | (hi[j] & ~mask);
        lo[0] |= take;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q[j] = lo[j];
        rem[j] = hi[j];
    }
}

// The division step on field elements in Montgomery form: with a and d read as canonical integers, *q = floor(a / d) and
// *rem = a mod d, both below the modulus, back in Montgomery form.  -> false, and nothing written, where d == 0.
template <class P>
PM_HD bool euclid_divrem(const Fp<P> &a, const Fp<P> &d, Fp<P> *q, Fp<P> *rem) {
    static_assert(P::N == 8, "four 64-bit words");
    if (d.is_zero()) return false;
    const Fp<P> ac = from_mont<P>(a), dc = from_mont<P>(d);
    uint64_t aw[4], dw[4], qw[4], rw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        aw[j] = (uint64_t)ac.l[2 * j] | (uint64_t)ac.l[2 * j + 1] << 32;
        dw[j] = (uint64_t)dc.l[2 * j] | (uint64_t)dc.l[2 * j + 1] << 32;
    }
    divrem256(aw, dw, qw, rw);
    Fp<P> qc, rc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        qc.l[2 * j] = (uint32_t)qw[j];
        qc.l[2 * j + 1] = (uint32_t)(qw[j] >> 32);
        rc.l[2 * j] = (uint32_t)rw[j];
        rc.l[2 * j + 1] = (uint32_t)(rw[j] >> 32);
    }
    *q = to_mont<P>(qc);
    *rem = to_mont<P>(rc);
    return true;
}

}  // namespace pm
